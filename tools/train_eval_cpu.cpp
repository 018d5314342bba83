// apd_trainer_evaluate as plain single-thread C++: the forward half of AutoEncoder::take_step
// (neural.rs:74-94) under frozen weights, operation for operation in f32 with the defined sigmoid of csrc/train_math.h, and
// main.rs:130's total as one f32 add per position.  Built under the sanitizers by tests/test_train_eval_reference.py it is a second
// witness of the checker's bits; at -O2 it is the CPU baseline of tools/train_eval_bench.py.  No HIP.
//   g++ -O2 -std=c++17 -ffp-contract=off tools/train_eval_cpu.cpp -o train_eval_cpu
//   train_eval_cpu run <case.bin>      per model: every error, the total (hex words) and the first non-finite position (-1: none)
//   train_eval_cpu bench <d_in> <latent> <n_frames> <repeats>    nanoseconds per position, best of <repeats> passes over random frames
// case.bin: u32 d_in, latent, n_models, n_frames, n_eval, order_per_model; per model w_encode, w_decode, b_encode, b_decode; frames;
// u32 order[rows][n_eval], rows = n_models with order_per_model, else 1.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../audio_pattern_discovery_amd/csrc/train_math.h"

struct EvalModel {
    uint32_t d, l;
    std::vector<float> we, wd, be, bd, latent;     // the reference's Mats: [d][l], [l][d], [l], [d]
    EvalModel(uint32_t d_in, uint32_t latent_) : d(d_in), l(latent_), we(d * l), wd(l * d), be(l), bd(d), latent(l) {}

    float error(const float *x)
    {
        float mn = INFINITY, mx = -INFINITY;                                   // Mat::norm (numerics.rs:192-208)
        for (uint32_t k = 0; k < d; ++k) {
            if (x[k] < mn && std::isfinite(x[k])) mn = x[k];
            if (x[k] > mx && std::isfinite(x[k])) mx = x[k];
        }
        const float scaler = mx - mn;
        const bool rescale = std::fabs(mn - mx) < 1e-8f;
        for (uint32_t j = 0; j < l; ++j) {
            float acc = 0.0f;
            for (uint32_t k = 0; k < d; ++k) acc = acc + x[k] * we[k * l + j];
            latent[j] = acc + be[j];
        }
        float dist = 0.0f;
        for (uint32_t i = 0; i < d; ++i) {
            float acc = 0.0f;
            for (uint32_t j = 0; j < l; ++j) acc = acc + latent[j] * wd[j * d + i];
            const float act = apd::train_sigmoid(acc + bd[i]);
            const float y = rescale ? (x[i] - mn) / scaler : x[i];
            const float diff = act - y;
            dist = dist + diff * diff;
        }
        return 0.5f * std::sqrt(dist);
    }
};

static uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static bool read_all(FILE *fp, void *dst, size_t bytes) { return bytes == 0 || std::fread(dst, 1, bytes, fp) == bytes; }

static int run_case(const char *path)
{
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return 2;
    uint32_t head[6];
    if (!read_all(fp, head, sizeof head) || head[0] == 0 || head[1] == 0 || head[0] > 64 || head[1] > 64 || head[2] == 0 || head[2] > 4096) { std::fclose(fp); return 2; }
    const uint32_t d = head[0], l = head[1], n_models = head[2], n_frames = head[3], n_eval = head[4], rows = head[5] ? n_models : 1;
    std::vector<EvalModel> models(n_models, EvalModel(d, l));
    bool ok = true;
    for (EvalModel &m : models)
        ok = ok && read_all(fp, m.we.data(), m.we.size() * 4) && read_all(fp, m.wd.data(), m.wd.size() * 4) && read_all(fp, m.be.data(), m.be.size() * 4) &&
             read_all(fp, m.bd.data(), m.bd.size() * 4);
    std::vector<float> frames((size_t)n_frames * d);
    std::vector<uint32_t> order((size_t)rows * n_eval);
    ok = ok && read_all(fp, frames.data(), frames.size() * 4) && read_all(fp, order.data(), order.size() * 4);
    std::fclose(fp);
    if (!ok) return 2;
    for (uint32_t i : order)
        if (i >= n_frames) return 2;
    for (uint32_t m = 0; m < n_models; ++m) {
        const uint32_t *row = order.data() + (size_t)(head[5] ? m : 0) * n_eval;
        float total = 0.0f;
        long long first = -1;
        for (uint32_t e = 0; e < n_eval; ++e) {
            const float err = models[m].error(frames.data() + (size_t)row[e] * d);
            std::printf("%08x\n", bits_of(err));
            total = total + err;
            if (first < 0 && !std::isfinite(err)) first = e;
        }
        std::printf("%08x\n%lld\n", bits_of(total), first);
    }
    return 0;
}

static int run_bench(uint32_t d, uint32_t l, uint32_t n_frames, int repeats)
{
    if (d == 0 || l == 0 || d > 64 || l > 64 || n_frames == 0) return 2;
    std::mt19937 rng(7);
    std::normal_distribution<float> gauss(0.0f, 2.0f);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    EvalModel m(d, l);
    for (float &w : m.we) w = (uni(rng) - 0.5f) / (float)l;
    for (float &w : m.wd) w = (uni(rng) - 0.5f) / (float)d;
    for (float &w : m.be) w = (uni(rng) - 0.5f) / (float)l;
    for (float &w : m.bd) w = (uni(rng) - 0.5f) / (float)d;
    std::vector<float> frames((size_t)n_frames * d);
    for (float &v : frames) v = gauss(rng);
    double best = 1e300, worst = 0.0;
    float total = 0.0f;
    for (int r = 0; r < repeats; ++r) {
        total = 0.0f;
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t i = 0; i < n_frames; ++i) total = total + m.error(frames.data() + (size_t)i * d);
        const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / n_frames;
        best = ns < best ? ns : best;
        worst = ns > worst ? ns : worst;
    }
    std::printf("{\"d_in\": %u, \"latent\": %u, \"frames\": %u, \"ns_per_position_best\": %.2f, \"ns_per_position_worst\": %.2f, \"total_err_bits\": \"%08x\"}\n", d,
                l, n_frames, best, worst, bits_of(total));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "run")) return run_case(argv[2]);
    if (argc == 6 && !std::strcmp(argv[1], "bench")) return run_bench((uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]), (uint32_t)std::atoi(argv[4]), std::atoi(argv[5]));
    std::fprintf(stderr, "usage: train_eval_cpu run <case.bin> | bench <d_in> <latent> <n_frames> <repeats>\n");
    return 1;
}
