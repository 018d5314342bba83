// The host-only entry points of the trainer (include/apd.h, "autoencoder training"): the learning-rate schedule and the order of
// an epoch.  Plain C++ like formats.hip: tools/train_cpu.cpp includes this unit and builds it without HIP, under the sanitizers.
#include <cmath>
#include <cstdint>

#include "../../include/apd.h"
#include "train_math.h"

// AutoEncoder::step_decay (neural.rs:26-28): learning_rate * drop ^ floor((1 + epoch) / epoch_drop), every operation in f32.
extern "C" float apd_step_decay(float learning_rate, float drop, float epoch_drop, float epoch)
{
    return learning_rate * powf(drop, floorf((1.0f + epoch) / epoch_drop));
}

// main.rs:120-124: the signals in order, each signal's frames in a fresh Fisher-Yates shuffle (rand's: i from the last position
// down to 1, swapped with a draw from [0, i]).  The draws come from train_math.h's counter-based generator, keyed by (seed, epoch,
// signal): the order is a function of the arguments alone.
extern "C" int apd_train_order(uint64_t seed, uint64_t epoch, const uint64_t *offsets, uint32_t n_seq, uint32_t *order)
{
    if (n_seq == 0) return APD_OK;
    if (!offsets) return APD_ERR_INVALID_ARG;
    for (uint32_t s = 0; s < n_seq; ++s)
        if (offsets[s + 1] < offsets[s]) return APD_ERR_INVALID_ARG;
    if (offsets[n_seq] >= (1ull << 32)) return APD_ERR_INVALID_ARG;        // the order holds 32-bit frame numbers
    if (offsets[n_seq] > offsets[0] && !order) return APD_ERR_INVALID_ARG;
    uint64_t at = 0;
    for (uint32_t s = 0; s < n_seq; ++s) {
        const uint64_t first = offsets[s], n = offsets[s + 1] - first;
        uint32_t *block = order + at;
        for (uint64_t i = 0; i < n; ++i) block[i] = (uint32_t)(first + i);
        const uint64_t key = apd::train_order_key(seed, epoch, s);
        for (uint64_t i = n; i-- > 1;) {
            const uint64_t j = apd::train_order_draw(key, i, i + 1);
            const uint32_t tmp = block[i];
            block[i] = block[j];
            block[j] = tmp;
        }
        at += n;
    }
    return APD_OK;
}
