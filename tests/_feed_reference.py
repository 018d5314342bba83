"""A numpy checker of the framing an apd_feed promises (include/apd.h, "raw audio in chunks"): which frames of a recording each push
emits, and what a channel carries from one push to the next.  Written from the reference's loop alone
(`for i in (fft_size..n).step_by(fft_step)`, spectrogram.rs:51; the frame is samples[i - fft_size .. i]), not from the library."""
import numpy as np


def frames_of(n, fft, step):
    """Frames of a recording of n samples: the length of range(fft, n, step)."""
    return len(range(fft, n, step))


class Channel:
    """One channel of a feed: `tail` samples kept from the start of the next window on, `skip` samples still to be dropped."""

    def __init__(self, fft, step):
        self.fft, self.step = fft, step
        self.samples = self.frames = self.tail = self.skip = 0

    def push(self, length):
        """Advances by a chunk of `length` samples; returns (first, last + 1) of the frames it emits."""
        first = self.frames
        self.samples += length
        self.frames = frames_of(self.samples, self.fft, self.step)
        window = self.frames * self.step                       # first sample of the next frame's window
        self.tail = max(self.samples - window, 0)
        self.skip = max(window - self.samples, 0)
        return first, self.frames


def pushes(fft, step, lengths):
    """The (first, last + 1) frame ranges a channel emits when it is fed chunks of these lengths, and the (tail, skip) after each."""
    c = Channel(fft, step)
    ranges, states = [], []
    for n in lengths:
        ranges.append(c.push(n))
        states.append((c.tail, c.skip))
    return ranges, states


def rows(whole, fft, step, lengths):
    """Given the frame matrix of the whole recording, the rows each push must return."""
    return [whole[a:b] for a, b in pushes(fft, step, lengths)[0]]


def random_split(rng, n, pieces, empty=0.2):
    """`pieces` chunk lengths that sum to n, some of them 0."""
    cuts = np.sort(rng.integers(0, n + 1, size=pieces - 1))
    for k in range(len(cuts)):
        if k and rng.random() < empty:
            cuts[k] = cuts[k - 1]
    return np.diff(np.concatenate([[0], cuts, [n]])).astype(int).tolist()
