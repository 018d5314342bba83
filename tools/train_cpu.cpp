// The trainer's step as plain single-thread C++: AutoEncoder::take_step (neural.rs:74-94) operation for
// operation in f32 with the defined sigmoid of csrc/train_math.h.  It is the CPU baseline of tools/train_bench.py (what a user of
// this library had before apd_trainer; NOT the Rust reference, which is not built here) and, built under the sanitizers by
// tests/test_train_reference.py, a second witness of the checker's bits.  Includes the host-only unit of the library: no HIP.
//   g++ -O2 -std=c++17 -ffp-contract=off tools/train_cpu.cpp -o train_cpu
//   train_cpu run <case.bin>            weights, total_err and first non-finite step after the case's steps, as hex words
//   train_cpu order <seed> <epoch> <offset>...      apd_train_order
//   train_cpu decay <lr> <drop> <epoch_drop> <epoch>    apd_step_decay, as a hex word
//   train_cpu bench <d_in> <latent> <n_frames> <repeats>   nanoseconds per step, best of <repeats> epochs over random frames
// case.bin: u32 d_in, latent, n_frames, n_steps; f32 alpha; w_encode, w_decode, b_encode, b_decode; frames; u32 order[n_steps].
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../audio_pattern_discovery_amd/csrc/train_host.hip"

struct CpuModel {
    uint32_t d, l;
    std::vector<float> we, wd, be, bd;     // the reference's Mats: [d][l], [l][d], [l], [d]
    float total_err = 0.0f;
    uint64_t steps = 0, first_nonfinite = ~0ull;
    std::vector<float> y, latent, la, act, dout, ddec;
    CpuModel(uint32_t d_in, uint32_t latent_) : d(d_in), l(latent_), we(d * l), wd(l * d), be(l), bd(d), y(d), latent(l), la(l), act(d), dout(d), ddec(l) {}

    void step(const float *x, float alpha)
    {
        float mn = INFINITY, mx = -INFINITY;                                   // Mat::norm (numerics.rs:192-208)
        for (uint32_t k = 0; k < d; ++k) {
            if (x[k] < mn && std::isfinite(x[k])) mn = x[k];
            if (x[k] > mx && std::isfinite(x[k])) mx = x[k];
        }
        const float scaler = mx - mn;
        const bool rescale = std::fabs(mn - mx) < 1e-8f;
        for (uint32_t k = 0; k < d; ++k) y[k] = rescale ? (x[k] - mn) / scaler : x[k];
        for (uint32_t j = 0; j < l; ++j) {
            float acc = 0.0f;
            for (uint32_t k = 0; k < d; ++k) acc = acc + x[k] * we[k * l + j];
            latent[j] = acc + be[j];
            la[j] = apd::train_sigmoid(latent[j]);
        }
        for (uint32_t i = 0; i < d; ++i) {
            float acc = 0.0f;
            for (uint32_t j = 0; j < l; ++j) acc = acc + latent[j] * wd[j * d + i];
            act[i] = apd::train_sigmoid(acc + bd[i]);
            dout[i] = ((y[i] - act[i]) * -1.0f) * (act[i] * (1.0f - act[i]));
        }
        for (uint32_t j = 0; j < l; ++j) {
            float acc = 0.0f;
            for (uint32_t i = 0; i < d; ++i) acc = acc + dout[i] * wd[j * d + i];
            ddec[j] = acc * (la[j] * (1.0f - la[j]));
        }
        bool finite = true;
        for (uint32_t j = 0; j < l; ++j)
            for (uint32_t i = 0; i < d; ++i) {
                wd[j * d + i] = wd[j * d + i] - (0.0f + latent[j] * dout[i]) * alpha;
                finite = finite && std::isfinite(wd[j * d + i]);
            }
        for (uint32_t k = 0; k < d; ++k)
            for (uint32_t j = 0; j < l; ++j) {
                we[k * l + j] = we[k * l + j] - (0.0f + x[k] * ddec[j]) * alpha;
                finite = finite && std::isfinite(we[k * l + j]);
            }
        for (uint32_t j = 0; j < l; ++j) { be[j] = be[j] - ddec[j] * alpha; finite = finite && std::isfinite(be[j]); }
        for (uint32_t i = 0; i < d; ++i) { bd[i] = bd[i] - dout[i] * alpha; finite = finite && std::isfinite(bd[i]); }
        float dist = 0.0f;
        for (uint32_t i = 0; i < d; ++i) { const float diff = act[i] - y[i]; dist = dist + diff * diff; }
        total_err = total_err + 0.5f * std::sqrt(dist);
        if (!finite && first_nonfinite == ~0ull) first_nonfinite = steps;
        ++steps;
    }
};

static uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static bool read_all(FILE *fp, void *dst, size_t bytes) { return bytes == 0 || std::fread(dst, 1, bytes, fp) == bytes; }

static int run_case(const char *path)
{
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return 2;
    uint32_t head[4];
    float alpha;
    if (!read_all(fp, head, sizeof head) || !read_all(fp, &alpha, 4) || head[0] == 0 || head[1] == 0 || head[0] > 64 || head[1] > 64) { std::fclose(fp); return 2; }
    CpuModel m(head[0], head[1]);
    std::vector<float> frames((size_t)head[2] * head[0]);
    std::vector<uint32_t> order(head[3]);
    const bool ok = read_all(fp, m.we.data(), m.we.size() * 4) && read_all(fp, m.wd.data(), m.wd.size() * 4) && read_all(fp, m.be.data(), m.be.size() * 4) &&
                    read_all(fp, m.bd.data(), m.bd.size() * 4) && read_all(fp, frames.data(), frames.size() * 4) && read_all(fp, order.data(), order.size() * 4);
    std::fclose(fp);
    if (!ok) return 2;
    for (uint32_t i : order) {
        if (i >= head[2]) return 2;
        m.step(frames.data() + (size_t)i * m.d, alpha);
    }
    for (const std::vector<float> *v : {&m.we, &m.wd, &m.be, &m.bd})
        for (float f : *v) std::printf("%08x\n", bits_of(f));
    std::printf("%08x\n%llu\n%lld\n", bits_of(m.total_err), (unsigned long long)m.steps, m.first_nonfinite == ~0ull ? -1ll : (long long)m.first_nonfinite);
    return 0;
}

static int run_bench(uint32_t d, uint32_t l, uint32_t n_frames, int repeats)
{
    if (d == 0 || l == 0 || d > 64 || l > 64 || n_frames == 0) return 2;
    std::mt19937 rng(7);
    std::normal_distribution<float> gauss(0.0f, 2.0f);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    CpuModel m(d, l);
    for (float &w : m.we) w = (uni(rng) - 0.5f) / (float)l;
    for (float &w : m.wd) w = (uni(rng) - 0.5f) / (float)d;
    for (float &w : m.be) w = (uni(rng) - 0.5f) / (float)l;
    for (float &w : m.bd) w = (uni(rng) - 0.5f) / (float)d;
    std::vector<float> frames((size_t)n_frames * d);
    for (float &v : frames) v = gauss(rng);
    const uint64_t offsets[2] = {0, n_frames};
    std::vector<uint32_t> order(n_frames);
    double best = 1e300, worst = 0.0;
    for (int r = 0; r < repeats; ++r) {
        if (apd_train_order(1, (uint64_t)r, offsets, 1, order.data()) != APD_OK) return 2;
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t i : order) m.step(frames.data() + (size_t)i * d, 0.1f);
        const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / n_frames;
        best = ns < best ? ns : best;
        worst = ns > worst ? ns : worst;
    }
    std::printf("{\"d_in\": %u, \"latent\": %u, \"frames\": %u, \"ns_per_step_best\": %.2f, \"ns_per_step_worst\": %.2f, \"total_err_bits\": \"%08x\"}\n", d, l,
                n_frames, best, worst, bits_of(m.total_err));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !std::strcmp(argv[1], "run")) return run_case(argv[2]);
    if (argc >= 4 && !std::strcmp(argv[1], "order")) {
        std::vector<uint64_t> offsets;
        for (int i = 4; i < argc; ++i) offsets.push_back(std::strtoull(argv[i], nullptr, 10));
        const uint32_t n_seq = offsets.empty() ? 0 : (uint32_t)offsets.size() - 1;
        std::vector<uint32_t> order(n_seq ? (size_t)(offsets.back() - offsets.front()) : 0);
        if (apd_train_order(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), offsets.data(), n_seq, order.data()) != APD_OK) return 3;
        for (uint32_t o : order) std::printf("%u\n", o);
        return 0;
    }
    if (argc == 6 && !std::strcmp(argv[1], "decay")) {
        std::printf("%08x\n", bits_of(apd_step_decay(std::strtof(argv[2], nullptr), std::strtof(argv[3], nullptr), std::strtof(argv[4], nullptr), std::strtof(argv[5], nullptr))));
        return 0;
    }
    if (argc == 6 && !std::strcmp(argv[1], "bench")) return run_bench((uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]), (uint32_t)std::atoi(argv[4]), std::atoi(argv[5]));
    std::fprintf(stderr, "usage: train_cpu run <case.bin> | order <seed> <epoch> <offset>... | decay <lr> <drop> <epoch_drop> <epoch> | bench <d_in> <latent> <n_frames> <repeats>\n");
    return 1;
}
