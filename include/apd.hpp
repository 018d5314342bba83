// apd.hpp -- header-only C++ mirror of the reference's Rust surface for the alignment/clustering path, over the C ABI
// of apd.h.  Names and argument meaning follow the Rust items (file:line cited at each); the compute is libapd_hip.so.
// Errors that are panics in the reference (zero-length sequence, percentile index out of range) throw apd::Error.
#pragma once
#include <algorithm>
#include <cstdint>
#include <fstream>
#include <iterator>
#include <limits>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "apd.h"

namespace apd {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string &what) : std::runtime_error(what), status(s) {}
};

inline void check(int status, apd_context *ctx = nullptr)
{
    if (status == APD_OK) return;
    std::string msg = apd_status_string(status);
    if (ctx && status == APD_ERR_HIP) msg += std::string(": ") + apd_last_error(ctx);
    throw Error(status, msg);
}

class Context {
  public:
    explicit Context(int device = 0) { check(apd_create(device, &ctx_)); }
    ~Context() { if (ctx_) apd_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    apd_context *get() const { return ctx_; }
    // 0 difference form, 1 hybrid (default), 2 strict: the Rust build's bits for every penalty set (apd.h, apd_set_distance_mode)
    void set_distance_mode(int mode, float tau = 0.0f) { check(apd_set_distance_mode(ctx_, mode, tau)); }
  private:
    apd_context *ctx_ = nullptr;
};

// spectrogram.rs:13-24 -- flat row-major frames [T][n_bins]
struct NDSequence {
    std::size_t n_bins = 0;
    std::vector<float> frames;
    std::size_t audio_id = 0;
    const float *vec(std::size_t t) const { return frames.data() + t * n_bins; }     // :99-101
    std::size_t len() const { return n_bins ? frames.size() / n_bins : 0; }         // :152-154
};

// numerics.rs:171-174
struct Mat {
    std::vector<float> flat;
    std::size_t cols = 0;
    std::size_t rows() const { return cols ? flat.size() / cols : 0; }
};

// neural.rs:12-71: the weight file and the forward pass (training is outside the accelerated path)
struct AutoEncoder {
    Mat w_encode, w_decode, b_encode, b_decode;
    std::size_t n_latent() const { return b_encode.cols; }                          // :22-24
    static AutoEncoder from_bytes(const std::vector<unsigned char> &buf)             // bincode::deserialize, :34
    {
        apd_autoencoder_view v;
        check(apd_autoencoder_parse(buf.data(), buf.size(), &v));
        AutoEncoder nn;
        const apd_mat_view *views[4] = {&v.w_encode, &v.w_decode, &v.b_encode, &v.b_decode};
        Mat *mats[4] = {&nn.w_encode, &nn.w_decode, &nn.b_encode, &nn.b_decode};
        for (int k = 0; k < 4; ++k) {
            mats[k]->flat.resize(views[k]->len);
            mats[k]->cols = views[k]->cols;
            check(apd_autoencoder_copy(buf.data(), views[k], mats[k]->flat.data()));
        }
        return nn;
    }
    static AutoEncoder from_file(const std::string &file)                            // :30-36
    {
        std::ifstream in(file, std::ios::binary);
        if (!in) throw Error(APD_ERR_INVALID_ARG, "cannot open " + file);            // File::open(file)? -> DiscoveryError::IO
        const std::vector<unsigned char> buf((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        return from_bytes(buf);
    }
    void save_file(const std::string &file) const                                    // :39-44
    {
        const uint32_t latent = (uint32_t)w_encode.cols, d_in = (uint32_t)w_encode.rows();
        uint64_t n = 0;
        check(apd_autoencoder_serialize(nullptr, nullptr, nullptr, nullptr, d_in, latent, nullptr, 0, &n));
        std::vector<unsigned char> buf(n);
        check(apd_autoencoder_serialize(w_encode.flat.data(), w_decode.flat.data(), b_encode.flat.data(), b_decode.flat.data(), d_in, latent,
                                        buf.data(), buf.size(), &n));
        std::ofstream out(file, std::ios::binary);
        out.write((const char *)buf.data(), (std::streamsize)buf.size());
        if (!out) throw Error(APD_ERR_INVALID_ARG, "cannot write " + file);
    }
    // AutoEncoder::predict on every frame of a sequence = NDSequence::encoded (neural.rs:55-71, spectrogram.rs:103-121)
    NDSequence encoded(Context &ctx, const NDSequence &x) const
    {
        if (x.n_bins != w_encode.rows()) throw Error(APD_ERR_INVALID_ARG, "self.cols == other.rows()");   // numerics.rs:306
        NDSequence out;
        out.n_bins = n_latent();
        out.audio_id = x.audio_id;
        out.frames.resize(x.len() * out.n_bins);
        check(apd_encode(ctx.get(), x.frames.data(), x.len(), (uint32_t)x.n_bins, w_encode.flat.data(), b_encode.flat.data(), (uint32_t)out.n_bins, 0,
                         out.frames.data()), ctx.get());
        return out;
    }
};

// alignments.rs:77-83
struct AlignmentParams {
    std::size_t warping_band;
    float insertion_penalty, deletion_penalty, match_penalty;
    static AlignmentParams default_for(std::size_t len) { return {len, 1.0f, 1.0f, 1.0f}; }   // :86-93
};

// discovery.rs:7-26 -- every field of project/config/Discovery.toml (defaults: the shipped file)
struct Discovery {
    std::size_t dft_win = 256, dft_step = 128, ceps_filter = 32, vat_moving = 15;
    float vat_percentile = 0.95f;
    std::size_t vat_min_len = 150;
    std::size_t alignment_workers = 4;      // accepted, unused: the GPU grid replaces the OS threads
    float clustering_percentile = 0.05f;
    float warping_band_percentage = 1.0f, insertion_penalty = 1.0f, deletion_penalty = 1.0f, match_penalty = 1.0f;
    std::size_t auto_encoder = 10;
    float learning_rate = 0.1f;
    std::size_t epochs = 25;
    float epoch_drop = 5.0f, drop = 0.5f;
    static Discovery from_toml(const std::string &file)                             // discovery.rs:28-36
    {
        std::ifstream in(file);
        if (!in) throw Error(APD_ERR_INVALID_ARG, "Template file not found");        // .expect() at :31
        const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        apd_discovery d;
        check(apd_discovery_parse_toml(text.c_str(), &d));                            // toml::from_str(..).unwrap() at :34
        Discovery c;
        c.dft_win = d.dft_win; c.dft_step = d.dft_step; c.ceps_filter = d.ceps_filter; c.vat_moving = d.vat_moving;
        c.vat_percentile = d.vat_percentile; c.vat_min_len = d.vat_min_len; c.alignment_workers = d.alignment_workers;
        c.clustering_percentile = d.clustering_percentile; c.warping_band_percentage = d.warping_band_percentage;
        c.insertion_penalty = d.insertion_penalty; c.deletion_penalty = d.deletion_penalty; c.match_penalty = d.match_penalty;
        c.auto_encoder = d.auto_encoder; c.learning_rate = d.learning_rate; c.epochs = d.epochs; c.epoch_drop = d.epoch_drop; c.drop = d.drop;
        return c;
    }
    apd_align_config config() const { return {warping_band_percentage, insertion_penalty, deletion_penalty, match_penalty}; }
    AlignmentParams alignment_params(std::size_t n_size) const                       // discovery.rs:38-45
    {
        const apd_align_config c = config();
        apd_alignment_params p;
        check(apd_discovery_alignment_params(&c, n_size, &p));
        return {(std::size_t)p.warping_band, p.insertion_penalty, p.deletion_penalty, p.match_penalty};
    }
};

// alignments.rs:99-181.  `sparse` is not materialised as a whole; path() returns the cells a reader of the table meets walking
// back from the score cell (n-1, m-1), with their table values and branches (apd.h, "warping paths").
class Alignment {
  public:
    explicit Alignment(Context &ctx) : ctx_(ctx) {}                                  // Alignment::new, :107-111
    std::size_t n = 0, m = 0;
    void construct_alignment(const NDSequence &x, const NDSequence &y, const AlignmentParams &p, bool with_path = false)   // :165-180
    {
        n = x.len(); m = y.len();
        const apd_alignment_params cp{(uint64_t)p.warping_band, p.insertion_penalty, p.deletion_penalty, p.match_penalty};
        const uint32_t dim = (uint32_t)(x.n_bins ? x.n_bins : y.n_bins);
        path_.clear();
        if (!with_path) {
            check(apd_align_pair(ctx_.get(), x.frames.data(), n, y.frames.data(), m, dim, &cp, &score_), ctx_.get());
            return;
        }
        path_.resize(std::max<uint64_t>(apd_path_bound(n, m), 1));
        uint64_t used = 0;
        check(apd_align_pair_path(ctx_.get(), x.frames.data(), n, y.frames.data(), m, dim, &cp, path_.data(), path_.size(), &used, &score_),
              ctx_.get());
        path_.resize(used);
    }
    float score() const { return (n == 0 && m == 0) ? std::numeric_limits<float>::infinity() : score_; }   // :116-125
    // the warping path of the last construct_alignment(.., with_path = true): origin first, end cell last
    const std::vector<apd_path_step> &path() const { return path_; }
  private:
    Context &ctx_;
    float score_ = std::numeric_limits<float>::infinity();
    std::vector<apd_path_step> path_;
};

// An apd_batch owned by the caller; Batch::join: the sequences of `first` followed by those of `second` in one resident batch
// (apd_batch_join), an ordinary batch for every call that takes one and what apd_align_cross aligns.
class Batch {
  public:
    explicit Batch(apd_batch *handle) : handle_(handle) {}
    static Batch join(Context &ctx, const apd_batch *first, const apd_batch *second)
    {
        apd_batch *j = nullptr;
        check(apd_batch_join(ctx.get(), first, second, &j), ctx.get());
        return Batch(j);
    }
    ~Batch() { if (handle_) apd_batch_destroy(handle_); }
    Batch(Batch &&o) noexcept : handle_(o.handle_) { o.handle_ = nullptr; }
    Batch(const Batch &) = delete;
    Batch &operator=(const Batch &) = delete;
    apd_batch *get() const { return handle_; }
    apd_batch *release() { apd_batch *h = handle_; handle_ = nullptr; return h; }
    uint32_t len() const { return apd_batch_len(handle_); }
    uint32_t first_len() const { return apd_batch_first_len(handle_); }
  private:
    apd_batch *handle_ = nullptr;
};

// Not in the reference: a streaming spotting session (apd.h, "streaming spotting"), made by AlignmentWorkers::spot_stream.  Pair p =
// channel * n_queries + q; the curves of the pushes, one after the other, are spot()'s curves of the whole stream, bit for bit.
class SpotStream {
  public:
    SpotStream(Context &ctx, const apd_batch *templates, uint32_t dim, const std::vector<uint32_t> &queries, const Discovery &params,
               uint32_t channels)
        : ctx_(ctx), dim_(dim), n_queries_((uint32_t)queries.size()), channels_(channels)
    {
        const apd_align_config c = params.config();
        check(apd_spot_stream_create(ctx_.get(), templates, &c, queries.data(), n_queries_, channels_, &handle_), ctx_.get());
    }
    ~SpotStream() { if (handle_) apd_spot_stream_destroy(handle_); }
    SpotStream(SpotStream &&o) noexcept : ctx_(o.ctx_), handle_(o.handle_), dim_(o.dim_), n_queries_(o.n_queries_), channels_(o.channels_) { o.handle_ = nullptr; }
    SpotStream(const SpotStream &) = delete;
    SpotStream &operator=(const SpotStream &) = delete;
    // chunks[k]: channel k's frames, [m_k][dim] packed, m_k = 0 allowed.  cost / start: per pair, one entry per pushed column (left
    // empty with with_curves = false); best: the running best per pair, columns absolute.
    struct Pushed { std::vector<std::vector<float>> cost; std::vector<std::vector<uint32_t>> start; std::vector<apd_spot_best> best; };
    Pushed push(const std::vector<std::vector<float>> &chunks, bool with_curves = true)
    {
        if (chunks.size() != channels_) throw Error(APD_ERR_INVALID_ARG, "one chunk per channel");
        std::vector<uint64_t> chunk_off(channels_ + 1, 0);
        std::vector<float> frames;
        for (uint32_t k = 0; k < channels_; ++k) {
            chunk_off[k + 1] = chunk_off[k] + chunks[k].size() / dim_;
            frames.insert(frames.end(), chunks[k].begin(), chunks[k].end());
        }
        const std::size_t n_pairs = (std::size_t)n_queries_ * channels_;
        std::vector<uint64_t> off(n_pairs + 1, 0);
        Pushed out;
        out.best.resize(n_pairs);
        if (!with_curves) {
            check(apd_spot_stream_push(ctx_.get(), handle_, frames.data(), chunk_off.data(), dim_, 0, nullptr, nullptr, 0, off.data(),
                                       out.best.data()), ctx_.get());
            return out;
        }
        std::vector<float> cost(std::max<uint64_t>(chunk_off.back() * n_queries_, 1));
        std::vector<uint32_t> start(cost.size());
        check(apd_spot_stream_push(ctx_.get(), handle_, frames.data(), chunk_off.data(), dim_, 0, cost.data(), start.data(), cost.size(),
                                   off.data(), out.best.data()), ctx_.get());
        for (std::size_t p = 0; p < n_pairs; ++p) {
            out.cost.emplace_back(cost.begin() + off[p], cost.begin() + off[p + 1]);
            out.start.emplace_back(start.begin() + off[p], start.begin() + off[p + 1]);
        }
        return out;
    }
    static constexpr uint32_t kAllChannels = 0xFFFFFFFFu;
    void reset(uint32_t channel = kAllChannels, uint64_t first_column = 0)
    {
        check(apd_spot_stream_reset(ctx_.get(), handle_, channel, first_column), ctx_.get());
    }
    uint64_t columns(uint32_t channel) const
    {
        uint64_t c = 0;
        check(apd_spot_stream_columns(handle_, channel, &c));
        return c;
    }
    // From now on the session keeps its last history_columns columns (0: none); windows inside them can be traced: paths().
    void keep(uint32_t history_columns) { check(apd_spot_stream_keep(ctx_.get(), handle_, history_columns), ctx_.get()); }
    // [first, last] of the channel's kept columns; first == last + 1: none.
    std::pair<uint64_t, uint64_t> history(uint32_t channel) const
    {
        uint64_t first = 0, last = 0;
        check(apd_spot_stream_history(handle_, channel, &first, &last));
        return {first, last};
    }
    // windows: x = index into the session's queries, y = channel, end / start absolute columns as push() reports them.  steps[p] is
    // empty for a window that has aged out of the history, for a {0, 0} record and for a start that is not the table's.
    struct Paths { std::vector<std::vector<apd_path_step>> steps; std::vector<uint32_t> found_start; std::vector<float> scores; };
    Paths paths(const std::vector<apd_spot_window> &windows)
    {
        const std::size_t k = windows.size();
        std::vector<uint64_t> off(k + 1, 0);
        std::vector<uint32_t> len(k, 0);
        Paths out;
        out.found_start.assign(k, 0);
        out.scores.assign(k, 0.0f);
        check(apd_spot_stream_paths(ctx_.get(), handle_, windows.data(), k, nullptr, 0, off.data(), nullptr, nullptr, nullptr), ctx_.get());   // sizes
        std::vector<apd_path_step> steps(std::max<uint64_t>(off.back(), 1));
        check(apd_spot_stream_paths(ctx_.get(), handle_, windows.data(), k, steps.data(), steps.size(), off.data(), len.data(),
                                    out.found_start.data(), out.scores.data()), ctx_.get());
        for (std::size_t p = 0; p < k; ++p) out.steps.emplace_back(steps.begin() + off[p], steps.begin() + off[p] + len[p]);
        return out;
    }
  private:
    Context &ctx_;
    apd_spot_stream *handle_ = nullptr;
    uint32_t dim_ = 1, n_queries_ = 0, channels_ = 1;
};

// alignments.rs:11-68
class AlignmentWorkers {
  public:
    AlignmentWorkers(Context &ctx, std::vector<NDSequence> data) : data(std::move(data)), ctx_(ctx)   // ::new, :17-26
    {
        const std::size_t n = this->data.size();
        result.assign(n * n, 0.0f);
        offsets.assign(n + 1, 0);
        dim = n ? (uint32_t)this->data[0].n_bins : 1;
        for (std::size_t s = 0; s < n; ++s) {
            if (this->data[s].n_bins != dim) throw Error(APD_ERR_INVALID_ARG, "sequences must share n_bins");
            offsets[s + 1] = offsets[s] + this->data[s].len();
            frames.insert(frames.end(), this->data[s].frames.begin(), this->data[s].frames.end());
        }
        if (dim == 0) dim = 1;
        check(apd_batch_create(ctx_.get(), frames.data(), offsets.data(), (uint32_t)n, dim, 0, &batch_), ctx_.get());
    }
    ~AlignmentWorkers()
    {
        if (multi_) apd_multi_destroy(multi_);                                       // also destroys its batch
        if (batch_) apd_batch_destroy(batch_);
    }
    AlignmentWorkers(const AlignmentWorkers &) = delete;
    AlignmentWorkers &operator=(const AlignmentWorkers &) = delete;
    void align_all(const Discovery &params)                                          // :31-67, blocking
    {
        const apd_align_config c = params.config();
        check(apd_align_all(ctx_.get(), batch_, &c, result.data()), ctx_.get());
    }
    // The same over several GPUs of one node (the reference's `alignment_workers` threads, alignments.rs:33-41, become devices):
    // pair tiles sharded over `devices`, one RCCL all-gather inside the library.  The multi-device handle (contexts,
    // communicators, worker threads, the corpus resident on every device) is made on the first call and kept: a host that calls
    // align_all in a loop (main.rs:187-195) pays setup once.  Returns the ranks RCCL saw.
    uint32_t align_all(const Discovery &params, const std::vector<int> &devices)
    {
        const apd_align_config c = params.config();
        if (multi_ && devices != multi_devices_) { apd_multi_destroy(multi_); multi_ = nullptr; multi_batch_ = nullptr; }
        if (!multi_) {
            check(apd_multi_create(devices.data(), (uint32_t)devices.size(), &multi_));
            multi_devices_ = devices;
            const int rc = apd_multi_batch_create(multi_, frames.data(), nullptr, offsets.data(), (uint32_t)data.size(), dim, &multi_batch_);
            if (rc != APD_OK) throw Error(rc, std::string(apd_status_string(rc)) + ": " + apd_multi_last_error(multi_));
        }
        const int rc = apd_multi_align_all(multi_, multi_batch_, &c, result.data());
        if (rc != APD_OK) throw Error(rc, std::string(apd_status_string(rc)) + ": " + apd_multi_last_error(multi_));
        uint32_t seen = 0;
        check(apd_multi_ranks_seen(multi_, &seen));
        return seen;
    }
    // Not in the reference: this object's sequences against `other`'s (same context): apd_batch_join + apd_align_cross.
    // fs[q * n2 + c] = score(x = data[q], y = other.data[c]); sf[c * n1 + q] = score(x = other.data[c], y = data[q]).
    std::pair<std::vector<float>, std::vector<float>> cross(const AlignmentWorkers &other, const Discovery &params)
    {
        const apd_align_config c = params.config();
        const std::size_t n1 = data.size(), n2 = other.data.size();
        std::pair<std::vector<float>, std::vector<float>> out{std::vector<float>(n1 * n2), std::vector<float>(n1 * n2)};
        Batch joined = Batch::join(ctx_, batch_, other.batch_);
        check(apd_align_cross(ctx_.get(), joined.get(), &c, out.first.data(), out.second.data()), ctx_.get());
        return out;
    }
    // Not in the reference: subsequence alignment (apd.h, "subsequence alignment").  pairs: (query, stream) in this object's sequence
    // numbers -- with `streams`, in those of the two joined: below data.size() this object's, the others `streams`'.  curves: per
    // pair the cost and start of every stream column (left empty with with_curves = false); best: the best window per pair.
    struct Spotted { std::vector<std::vector<float>> cost; std::vector<std::vector<uint32_t>> start; std::vector<apd_spot_best> best; };
    Spotted spot(const std::vector<std::pair<uint32_t, uint32_t>> &pairs, const Discovery &params, bool with_curves = true,
                 const AlignmentWorkers *streams = nullptr)
    {
        const apd_align_config c = params.config();
        std::vector<uint32_t> flat;
        for (const auto &p : pairs) { flat.push_back(p.first); flat.push_back(p.second); }
        Batch joined(streams ? Batch::join(ctx_, batch_, streams->batch_).release() : nullptr);
        const apd_batch *b = streams ? joined.get() : batch_;
        std::vector<uint64_t> off(pairs.size() + 1, 0);
        Spotted out;
        out.best.resize(pairs.size());
        if (!with_curves) {
            check(apd_spot(ctx_.get(), b, &c, flat.data(), pairs.size(), nullptr, nullptr, 0, off.data(), out.best.data()), ctx_.get());
            return out;
        }
        check(apd_spot(ctx_.get(), b, &c, flat.data(), pairs.size(), nullptr, nullptr, 0, off.data(), nullptr), ctx_.get());   // sizes
        std::vector<float> cost(std::max<uint64_t>(off.back(), 1));
        std::vector<uint32_t> start(cost.size());
        check(apd_spot(ctx_.get(), b, &c, flat.data(), pairs.size(), cost.data(), start.data(), cost.size(), off.data(), out.best.data()), ctx_.get());
        for (std::size_t p = 0; p < pairs.size(); ++p) {
            out.cost.emplace_back(cost.begin() + off[p], cost.begin() + off[p + 1]);
            out.start.emplace_back(start.begin() + off[p], start.begin() + off[p + 1]);
        }
        return out;
    }
    // Not in the reference: the warping paths of spotted windows (apd.h, "warping paths of spotted windows").  windows: x, y numbered as
    // spot()'s pairs, end and start as Spotted::best or spot_hits() reported them; a pair may appear once per hit.  steps[k]: origin
    // first, (n, end) last; empty for a {0, 0} window and for a start that is not the table's -- found_start[k] then says which
    // start to ask again with.
    struct SpotPaths { std::vector<std::vector<apd_path_step>> steps; std::vector<uint32_t> found_start; std::vector<float> scores; };
    SpotPaths spot_paths(const std::vector<apd_spot_window> &windows, const Discovery &params, const AlignmentWorkers *streams = nullptr)
    {
        const apd_align_config c = params.config();
        Batch joined(streams ? Batch::join(ctx_, batch_, streams->batch_).release() : nullptr);
        const apd_batch *b = streams ? joined.get() : batch_;
        const std::size_t k = windows.size();
        std::vector<uint64_t> off(k + 1, 0);
        std::vector<uint32_t> len(k, 0);
        SpotPaths out;
        out.found_start.resize(k);
        out.scores.resize(k);
        check(apd_spot_paths(ctx_.get(), b, &c, windows.data(), k, nullptr, 0, off.data(), nullptr, nullptr, nullptr), ctx_.get());   // sizes
        std::vector<apd_path_step> steps(std::max<uint64_t>(off.back(), 1));
        check(apd_spot_paths(ctx_.get(), b, &c, windows.data(), k, steps.data(), steps.size(), off.data(), len.data(), out.found_start.data(),
                             out.scores.data()), ctx_.get());
        for (std::size_t p = 0; p < k; ++p) out.steps.emplace_back(steps.begin() + off[p], steps.begin() + off[p] + len[p]);
        return out;
    }
    // Not in the reference: streaming spotting (apd.h, "streaming spotting").  queries: this object's sequence numbers, repeats
    // allowed; this object must outlive the session.
    SpotStream spot_stream(const std::vector<uint32_t> &queries, const Discovery &params, uint32_t channels = 1)
    {
        return SpotStream(ctx_, batch_, dim, queries, params, channels);
    }
    // Not in the reference: DTW barycenter averaging (apd.h, "cluster prototypes") of the sets of this object's sequence numbers in
    // `sets`; init[k]: the sequence whose frames start set k's barycenter (usually AgglomerativeClustering::medoids' choice).
    // frames[k]: [T_k][dim] packed, T_k the length of init[k] (0 for an empty set); inertia / used: [iterations][sets.size()].
    struct Barycenters { std::vector<std::vector<float>> frames; std::vector<float> inertia; std::vector<uint32_t> used; };
    Barycenters barycenters(const std::vector<std::vector<std::size_t>> &sets, const std::vector<uint32_t> &init, const Discovery &params,
                            uint32_t iterations = 10)
    {
        if (init.size() != sets.size()) throw Error(APD_ERR_INVALID_ARG, "one init sequence per set");
        const apd_align_config c = params.config();
        std::vector<uint32_t> members, off(1, 0u);
        for (const auto &s : sets) { members.insert(members.end(), s.begin(), s.end()); off.push_back((uint32_t)members.size()); }
        const uint32_t n_sets = (uint32_t)sets.size();
        std::vector<uint64_t> frame_off(sets.size() + 1, 0);
        check(apd_barycenters(ctx_.get(), batch_, &c, members.data(), off.data(), n_sets, init.data(), iterations, nullptr, 0, 0,
                              frame_off.data(), nullptr, nullptr), ctx_.get());                                          // sizes
        std::vector<float> flat(std::max<uint64_t>(frame_off.back() * dim, 1));
        Barycenters out{{}, std::vector<float>((std::size_t)iterations * n_sets), std::vector<uint32_t>((std::size_t)iterations * n_sets)};
        check(apd_barycenters(ctx_.get(), batch_, &c, members.data(), off.data(), n_sets, init.data(), iterations, flat.data(), 0,
                              frame_off.back(), frame_off.data(), out.inertia.data(), out.used.data()), ctx_.get());
        for (std::size_t k = 0; k < sets.size(); ++k) out.frames.emplace_back(flat.begin() + frame_off[k] * dim, flat.begin() + frame_off[k + 1] * dim);
        return out;
    }
    const char *collective() const { return multi_ ? apd_multi_collective(multi_) : "none (one device)"; }
    std::vector<NDSequence> data;
    std::vector<float> result;                                                       // n*n row-major, diagonal 0.0
  private:
    Context &ctx_;
    apd_batch *batch_ = nullptr;
    apd_multi *multi_ = nullptr;                                                     // made by the first multi-device align_all
    apd_multi_batch *multi_batch_ = nullptr;
    std::vector<int> multi_devices_;
    std::vector<float> frames;                                                       // packed [sum len][dim], kept for the multi-device entry
    std::vector<uint64_t> offsets;
    uint32_t dim = 1;
};

// apd_spot_hits: the non-overlapping windows of one pair's curves whose score is strictly below `threshold`, best first.  Host only.
inline std::vector<apd_spot_best> spot_hits(const std::vector<float> &cost, const std::vector<uint32_t> &start, std::size_t n, float threshold)
{
    if (cost.size() != start.size()) throw Error(APD_ERR_INVALID_ARG, "cost and start are the two curves of one pair");
    uint64_t count = 0;
    check(apd_spot_hits(cost.data(), start.data(), cost.size(), n, threshold, nullptr, 0, &count));
    std::vector<apd_spot_best> hits(count);
    check(apd_spot_hits(cost.data(), start.data(), cost.size(), n, threshold, hits.data(), hits.size(), &count));
    return hits;
}

enum class Merge { Sequence2Sequence = 0, Sequence2Cluster = 1, Cluster2Sequence = 2, Cluster2Cluster = 3 };   // clustering.rs:8-13
struct ClusteringOperation { std::size_t merge_i, merge_j, into; float distance; Merge operation; };              // :19-25

struct AgglomerativeClustering {
    // clustering.rs:81-110
    static std::pair<std::vector<ClusteringOperation>, std::set<std::size_t>> clustering(Context &ctx, const std::vector<float> &distances,
                                                                                            std::size_t n_instances, float perc)
    {
        std::vector<apd_cluster_op> ops(n_instances ? n_instances : 1);
        std::vector<uint32_t> roots(n_instances ? n_instances : 1);
        uint32_t n_ops = 0, n_roots = 0;
        float thr = 0.0f;
        check(apd_clustering(ctx.get(), distances.data(), 0, (uint32_t)n_instances, perc, ops.data(), &n_ops, roots.data(), &n_roots, &thr),
              ctx.get());
        std::vector<ClusteringOperation> out;
        for (uint32_t t = 0; t < n_ops; ++t)
            out.push_back({ops[t].merge_i, ops[t].merge_j, ops[t].into, ops[t].distance, (Merge)ops[t].operation});
        return {out, std::set<std::size_t>(roots.begin(), roots.begin() + n_roots)};
    }
    // clustering.rs:40-76
    static std::vector<std::vector<std::size_t>> cluster_sets(const std::vector<ClusteringOperation> &operations,
                                                              const std::set<std::size_t> &cluster_ids, std::size_t n_instances)
    {
        std::vector<apd_cluster_op> ops;
        for (const auto &o : operations) ops.push_back({(uint32_t)o.merge_i, (uint32_t)o.merge_j, (uint32_t)o.into, o.distance, (uint32_t)o.operation});
        std::vector<uint32_t> roots(cluster_ids.begin(), cluster_ids.end()), members(n_instances + ops.size() + 2), off(roots.size() + 2);
        uint32_t n_sets = 0;
        check(apd_cluster_sets(ops.data(), (uint32_t)ops.size(), roots.data(), (uint32_t)roots.size(), (uint32_t)n_instances, members.data(),
                               off.data(), &n_sets));
        std::vector<std::vector<std::size_t>> out;
        for (uint32_t s = 0; s < n_sets; ++s) out.emplace_back(members.begin() + off[s], members.begin() + off[s + 1]);
        return out;
    }
    // Not in the reference: clustering.rs:153-170 between every first-set sequence (a cluster of its own) and every set of second-set
    // sequence numbers in `sets`, from the cross matrices of AlignmentWorkers::cross (apd_cross_linkage).
    struct CrossLinkage { std::vector<float> link_fs, link_sf; std::vector<uint32_t> nearest; std::vector<float> nearest_linkage; };
    static CrossLinkage cross_linkage(Context &ctx, const std::vector<float> &fs, const std::vector<float> &sf, std::size_t n_first,
                                      std::size_t n_second, const std::vector<std::vector<std::size_t>> &sets)
    {
        std::vector<uint32_t> members, off(1, 0u);
        for (const auto &s : sets) { members.insert(members.end(), s.begin(), s.end()); off.push_back((uint32_t)members.size()); }
        CrossLinkage r{std::vector<float>(n_first * sets.size()), std::vector<float>(n_first * sets.size()), std::vector<uint32_t>(n_first),
                       std::vector<float>(n_first)};
        check(apd_cross_linkage(ctx.get(), fs.data(), sf.data(), 0, (uint32_t)n_first, (uint32_t)n_second, members.data(), off.data(),
                                (uint32_t)sets.size(), r.link_fs.data(), r.link_sf.data(), r.nearest.data(), r.nearest_linkage.data()), ctx.get());
        return r;
    }
    // Not in the reference: the medoid of every set of `sets` from the n x n matrix of AlignmentWorkers::align_all
    // (apd_cluster_medoids): the smallest sequence number among the members of least cost, 0xFFFFFFFF / +INF if there is none.
    static std::pair<std::vector<uint32_t>, std::vector<float>> medoids(Context &ctx, const std::vector<float> &distances, std::size_t n_instances,
                                                                        const std::vector<std::vector<std::size_t>> &sets)
    {
        std::vector<uint32_t> members, off(1, 0u);
        for (const auto &s : sets) { members.insert(members.end(), s.begin(), s.end()); off.push_back((uint32_t)members.size()); }
        std::pair<std::vector<uint32_t>, std::vector<float>> r{std::vector<uint32_t>(sets.size()), std::vector<float>(sets.size())};
        check(apd_cluster_medoids(ctx.get(), distances.data(), 0, (uint32_t)n_instances, members.data(), off.data(), (uint32_t)sets.size(),
                                  r.first.data(), r.second.data()), ctx.get());
        return r;
    }
};

// Templates::dendrograms (reporting.rs:135-169), the strings: root id -> "[.k [<left> <right> ] ]" with leaf i rendered as
// labels[i]; roots no op made are absent (reporting.rs:200).
inline std::map<std::size_t, std::string> dendrograms(const std::vector<ClusteringOperation> &operations, const std::set<std::size_t> &clusters,
                                                      const std::vector<std::string> &labels)
{
    std::vector<apd_cluster_op> ops;
    for (const auto &o : operations) ops.push_back({(uint32_t)o.merge_i, (uint32_t)o.merge_j, (uint32_t)o.into, o.distance, (uint32_t)o.operation});
    const std::vector<uint32_t> roots(clusters.begin(), clusters.end());
    std::vector<const char *> lab;
    for (const auto &l : labels) lab.push_back(l.c_str());
    uint64_t bytes = 0;
    uint32_t n_strings = 0;
    std::vector<uint32_t> which(roots.size() + 1);
    check(apd_dendrograms(ops.data(), (uint32_t)ops.size(), roots.data(), (uint32_t)roots.size(), lab.data(), (uint32_t)lab.size(), nullptr, 0, &bytes,
                          which.data(), &n_strings));
    std::vector<char> buf(bytes + 1);
    check(apd_dendrograms(ops.data(), (uint32_t)ops.size(), roots.data(), (uint32_t)roots.size(), lab.data(), (uint32_t)lab.size(), buf.data(), bytes,
                          &bytes, which.data(), &n_strings));
    std::map<std::size_t, std::string> out;
    const char *p = buf.data();
    for (uint32_t i = 0; i < n_strings; ++i) { out[roots[which[i]]] = p; p += out[roots[which[i]]].size() + 1; }
    return out;
}

}  // namespace apd
