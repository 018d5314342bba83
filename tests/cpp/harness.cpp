// C++ harness over include/apd.hpp: reads a batch (text), runs the reference's main.rs:187-203 sequence through the
// C++ mirror -- AlignmentWorkers::new -> align_all -> AgglomerativeClustering::clustering -> cluster_sets -- and prints
// the results for tests/test_gpu_cpp_mirror.py to compare with the oracle.
//   usage: harness <input.txt>    input: n dim pct ins del match perc, then per sequence: len, then len*dim floats
//          harness <input.txt> <auto_encoder.bin> <Discovery.toml>   the same with the reference's on-disk artefacts: the
//              parameters come from the TOML file, every sequence goes through AutoEncoder::from_file(..) -> encoded() first
//              (main.rs:142-161), and the weight file is written back with save_file and compared byte for byte
//          harness <mode> <input.txt>   the wrappers that are not in the reference, compared bit for bit with the CPU checkers.
// Input of every mode: `pct ins del match dim`, the set A and -- in every mode but paths and stream -- the set B, then the mode's
// commands until the end of the file.  A set: `n`, then per sequence `len` and its len*dim values.  Every f32 is read and
// printed as the 8 hex digits of its bits; a step is `step i j costbits op`, a best record `best end start costbits scorebits`;
// a list of sets is `k`, then per set `size` and its members; a list of windows `k`, then per window `x y end start`.
//   mode        objects                                  commands (one result block each, in input order)
//   paths       one Alignment                            `x y`: construct_alignment(A[x], A[y], alignment_params(max len), true),
//                                                          path(), score()
//   cross       workers on A and on B, one context       none: cross(); Batch::join of two batches made through the C ABI with
//                                                          len(), first_len() and apd_align_cross on it; cross() again after the
//                                                          joined batch is gone
//   spot        workers on A, on B and on A + B          `spot <curves> <streams> k, k pairs x y`: spot() -- streams = 1: A's
//                                                          workers with B's as `streams`, 0: the workers on A + B, same numbers
//                                                        `hits <pair> <n> <threshold>`: spot_hits() on that pair's last curves
//                                                        `paths <streams> <from_hits> [x y] <windows>`: spot_paths() of one
//                                                          window (x, y) per last hit (from_hits = 1), then the listed ones
//   stream      workers on A; then `nq q.. channels`:    `push <curves> m_0 .. m_c-1, the frames`: push(), then columns()
//               spot_stream(), returned by value         `reset <channel> <first_column>`, `keep <H>`, `history`,
//                                                        `paths <windows>`
//   prototypes  workers on A (align_all) and on B        `medoids <sets>`: medoids() on A's result; `bary <iterations> <sets> k
//                                                          inits`: barycenters(); `linkage <sets>`: cross_linkage on cross()
// `refusal` in front of a command: an apd::Error prints `error <status> <text>` and the next command runs; otherwise it ends the
// run with exit code 1, as in the two reference forms.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

#include "../../include/apd.hpp"

namespace {

uint32_t bits_of(float v) { uint32_t b; std::memcpy(&b, &v, sizeof b); return b; }

// The text input of a mode: the header line, then whatever the mode reads from it.
struct Input {
    std::ifstream in;
    apd::Discovery cfg;
    std::size_t dim = 0;
    explicit Input(const char *file) : in(file)
    {
        cfg.warping_band_percentage = f32(); cfg.insertion_penalty = f32(); cfg.deletion_penalty = f32(); cfg.match_penalty = f32();
        in >> dim;
    }
    float f32()
    {
        std::string t;
        in >> t;
        const uint32_t b = (uint32_t)std::strtoul(t.c_str(), nullptr, 16);
        float v;
        std::memcpy(&v, &b, sizeof v);
        return v;
    }
    std::vector<float> frames(std::size_t count)
    {
        std::vector<float> out(count);
        for (auto &v : out) v = f32();
        return out;
    }
    std::vector<apd::NDSequence> set()
    {
        std::size_t n = 0;
        in >> n;
        std::vector<apd::NDSequence> seqs(n);
        for (auto &s : seqs) {
            std::size_t len = 0;
            in >> len;
            s.n_bins = dim;
            s.frames = frames(len * dim);
        }
        return seqs;
    }
    std::vector<std::vector<std::size_t>> sets()
    {
        std::size_t k = 0;
        in >> k;
        std::vector<std::vector<std::size_t>> out(k);
        for (auto &s : out) {
            std::size_t size = 0;
            in >> size;
            s.resize(size);
            for (auto &m : s) in >> m;
        }
        return out;
    }
    std::vector<uint32_t> u32s()
    {
        std::size_t k = 0;
        in >> k;
        std::vector<uint32_t> out(k);
        for (auto &v : out) in >> v;
        return out;
    }
    std::vector<apd_spot_window> windows()
    {
        std::size_t k = 0;
        in >> k;
        std::vector<apd_spot_window> out(k);
        for (auto &w : out) in >> w.x >> w.y >> w.end >> w.start;
        return out;
    }
};

void print_f32(const char *key, const std::vector<float> &values)
{
    std::printf("%s", key);
    for (float v : values) std::printf(" %08x", bits_of(v));
    std::printf("\n");
}

void print_u32(const char *key, const std::vector<uint32_t> &values)
{
    std::printf("%s", key);
    for (uint32_t v : values) std::printf(" %u", v);
    std::printf("\n");
}

void print_best(const apd_spot_best &b) { std::printf("best %u %u %08x %08x\n", b.end, b.start, bits_of(b.cost), bits_of(b.score)); }

void print_steps(const std::vector<apd_path_step> &steps)
{
    for (const auto &s : steps) std::printf("step %u %u %08x %u\n", s.i, s.j, bits_of(s.cost), s.op);
}

// Spotted and Pushed: `<key> <pairs> <pairs with curves>`, a best per pair, then cost and start per pair with curves
template <class R> void print_spotted(const char *key, const R &r)
{
    std::printf("%s %zu %zu\n", key, r.best.size(), r.cost.size());
    for (const auto &b : r.best) print_best(b);
    for (std::size_t p = 0; p < r.cost.size(); ++p) { print_f32("cost", r.cost[p]); print_u32("start", r.start[p]); }
}

// SpotPaths and Paths: `paths <windows>`, then per window `window found_start scorebits steps` and its steps
template <class R> void print_paths(const R &r)
{
    std::printf("paths %zu\n", r.steps.size());
    for (std::size_t p = 0; p < r.steps.size(); ++p) {
        std::printf("window %u %08x %zu\n", r.found_start[p], bits_of(r.scores[p]), r.steps[p].size());
        print_steps(r.steps[p]);
    }
}

// The commands of a mode, one after the other; run(cmd) returns false for a word it does not know.
template <class F> int commands(Input &io, F run)
{
    std::string cmd;
    bool refusal = false;
    while (io.in >> cmd) {
        if (cmd == "refusal") { refusal = true; continue; }
        try {
            if (!run(cmd)) { std::printf("unknown command %s\n", cmd.c_str()); return 2; }
        } catch (const apd::Error &e) {
            std::printf("error %d %s\n", e.status, e.what());
            if (!refusal) return 1;
        }
        refusal = false;
    }
    return 0;
}

int mode_paths(Input &io)
{
    apd::Context ctx(0);
    const auto a = io.set();
    apd::Alignment alignment(ctx);                                             // ONE object for every pair: path_ shrinks and grows
    return commands(io, [&](const std::string &cmd) {
        if (cmd != "pair") return false;
        std::size_t x = 0, y = 0;
        io.in >> x >> y;
        alignment.construct_alignment(a.at(x), a.at(y), io.cfg.alignment_params(std::max(a.at(x).len(), a.at(y).len())), true);
        std::printf("pair %zu %zu %zu %zu %08x %zu\n", x, y, alignment.n, alignment.m, bits_of(alignment.score()), alignment.path().size());
        print_steps(alignment.path());
        return true;
    });
}

apd::Batch make_batch(apd::Context &ctx, const std::vector<apd::NDSequence> &seqs, std::size_t dim)
{
    std::vector<float> frames;
    std::vector<uint64_t> offsets(1, 0);
    for (const auto &s : seqs) { frames.insert(frames.end(), s.frames.begin(), s.frames.end()); offsets.push_back(offsets.back() + s.len()); }
    apd_batch *handle = nullptr;
    apd::check(apd_batch_create(ctx.get(), frames.data(), offsets.data(), (uint32_t)seqs.size(), (uint32_t)dim, 0, &handle), ctx.get());
    return apd::Batch(handle);
}

int mode_cross(Input &io)
{
    apd::Context ctx(0);
    ctx.set_distance_mode(1);                                                  // the default, said through the wrapper; tau stays
    const auto a = io.set(), b = io.set();
    apd::AlignmentWorkers first(ctx, a), second(ctx, b);
    auto r = first.cross(second, io.cfg);
    print_f32("fs", r.first);
    print_f32("sf", r.second);
    {
        apd::Batch ba = make_batch(ctx, a, io.dim), bb = make_batch(ctx, b, io.dim);
        {
            apd::Batch joined = apd::Batch::join(ctx, ba.get(), bb.get());
            std::printf("join %u %u\n", joined.len(), joined.first_len());
            const apd_align_config c = io.cfg.config();
            std::vector<float> fs(a.size() * b.size()), sf(a.size() * b.size());
            apd::check(apd_align_cross(ctx.get(), joined.get(), &c, fs.data(), sf.data()), ctx.get());
            print_f32("direct_fs", fs);
            print_f32("direct_sf", sf);
        }
        std::printf("parts %u %u %u %u\n", ba.len(), ba.first_len(), bb.len(), bb.first_len());   // the inputs outlive the joined batch
    }
    r = first.cross(second, io.cfg);                                           // the first call's joined batch is long gone
    print_f32("again_fs", r.first);
    print_f32("again_sf", r.second);
    return 0;
}

int mode_spot(Input &io)
{
    apd::Context ctx(0);
    const auto a = io.set(), b = io.set();
    auto both = a;
    both.insert(both.end(), b.begin(), b.end());
    apd::AlignmentWorkers first(ctx, a), second(ctx, b), all(ctx, both);
    apd::AlignmentWorkers::Spotted last;
    std::vector<apd_spot_best> hits;
    return commands(io, [&](const std::string &cmd) {
        if (cmd == "spot") {
            int curves = 0, streams = 0;
            std::size_t k = 0;
            io.in >> curves >> streams >> k;
            std::vector<std::pair<uint32_t, uint32_t>> pairs(k);
            for (auto &p : pairs) io.in >> p.first >> p.second;
            last = streams ? first.spot(pairs, io.cfg, curves != 0, &second) : all.spot(pairs, io.cfg, curves != 0);
            print_spotted("spot", last);
        } else if (cmd == "hits") {
            std::size_t p = 0, n = 0;
            io.in >> p >> n;
            const float threshold = io.f32();
            hits = apd::spot_hits(last.cost.at(p), last.start.at(p), n, threshold);
            std::printf("hits %zu\n", hits.size());
            for (const auto &h : hits) print_best(h);
        } else if (cmd == "paths") {
            int streams = 0, from_hits = 0;
            uint32_t x = 0, y = 0;
            io.in >> streams >> from_hits;
            if (from_hits) io.in >> x >> y;
            std::vector<apd_spot_window> windows;
            if (from_hits)
                for (const auto &h : hits) windows.push_back({x, y, h.end, h.start});
            const auto listed = io.windows();
            windows.insert(windows.end(), listed.begin(), listed.end());
            print_paths(streams ? first.spot_paths(windows, io.cfg, &second) : all.spot_paths(windows, io.cfg));
        } else {
            return false;
        }
        return true;
    });
}

// By value, through a second object: the move constructor runs, and the destructor of an object that was moved from.
apd::SpotStream open_stream(apd::AlignmentWorkers &workers, const std::vector<uint32_t> &queries, const apd::Discovery &cfg, uint32_t channels)
{
    apd::SpotStream made = workers.spot_stream(queries, cfg, channels);
    apd::SpotStream moved(std::move(made));
    return moved;
}

int mode_stream(Input &io)
{
    apd::Context ctx(0);
    apd::AlignmentWorkers workers(ctx, io.set());
    const auto queries = io.u32s();
    uint32_t channels = 0;
    io.in >> channels;
    apd::SpotStream stream = open_stream(workers, queries, io.cfg, channels);
    auto print_columns = [&] {
        std::printf("columns");
        for (uint32_t k = 0; k < channels; ++k) std::printf(" %llu", (unsigned long long)stream.columns(k));
        std::printf("\n");
    };
    return commands(io, [&](const std::string &cmd) {
        if (cmd == "push") {
            int curves = 0;
            io.in >> curves;
            std::vector<std::size_t> len(channels);
            for (auto &m : len) io.in >> m;
            std::vector<std::vector<float>> chunks;
            for (std::size_t m : len) chunks.push_back(io.frames(m * io.dim));
            print_spotted("push", stream.push(chunks, curves != 0));
            print_columns();
        } else if (cmd == "reset") {
            uint32_t channel = 0;
            uint64_t first_column = 0;
            io.in >> channel >> first_column;
            stream.reset(channel, first_column);
            print_columns();
        } else if (cmd == "keep") {
            uint32_t history = 0;
            io.in >> history;
            stream.keep(history);
        } else if (cmd == "history") {
            for (uint32_t k = 0; k < channels; ++k) {
                const auto h = stream.history(k);
                std::printf("history %u %llu %llu\n", k, (unsigned long long)h.first, (unsigned long long)h.second);
            }
        } else if (cmd == "paths") {
            const auto windows = io.windows();
            print_paths(stream.paths(windows));
        } else {
            return false;
        }
        return true;
    });
}

int mode_prototypes(Input &io)
{
    apd::Context ctx(0);
    const auto a = io.set(), b = io.set();
    apd::AlignmentWorkers first(ctx, a), second(ctx, b);
    first.align_all(io.cfg);
    print_f32("dist", first.result);
    const auto cross = first.cross(second, io.cfg);
    print_f32("fs", cross.first);
    print_f32("sf", cross.second);
    return commands(io, [&](const std::string &cmd) {
        if (cmd == "medoids") {
            const auto sets = io.sets();
            const auto r = apd::AgglomerativeClustering::medoids(ctx, first.result, a.size(), sets);
            print_u32("medoid", r.first);
            print_f32("cost", r.second);
        } else if (cmd == "bary") {
            uint32_t iterations = 0;
            io.in >> iterations;
            const auto sets = io.sets();
            const auto init = io.u32s();
            const auto r = first.barycenters(sets, init, io.cfg, iterations);
            std::printf("bary %zu\n", r.frames.size());
            for (const auto &f : r.frames) print_f32("frames", f);
            print_f32("inertia", r.inertia);
            print_u32("used", r.used);
        } else if (cmd == "linkage") {
            const auto sets = io.sets();
            const auto r = apd::AgglomerativeClustering::cross_linkage(ctx, cross.first, cross.second, a.size(), b.size(), sets);
            print_f32("link_fs", r.link_fs);
            print_f32("link_sf", r.link_sf);
            print_u32("nearest", r.nearest);
            print_f32("nearest_linkage", r.nearest_linkage);
        } else {
            return false;
        }
        return true;
    });
}

struct Mode { const char *name; int (*run)(Input &); };
const Mode kModes[] = {{"paths", mode_paths}, {"cross", mode_cross}, {"spot", mode_spot}, {"stream", mode_stream}, {"prototypes", mode_prototypes}};

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    for (const Mode &mode : kModes) {
        if (argc != 3 || std::strcmp(argv[1], mode.name) != 0) continue;
        try {
            Input io(argv[2]);
            if (!io.in) { std::printf("cannot read %s\n", argv[2]); return 2; }
            return mode.run(io);
        } catch (const apd::Error &e) {
            std::printf("error %d %s\n", e.status, e.what());
            return 1;
        }
    }
    std::ifstream in(argv[1]);
    std::size_t n, dim;
    apd::Discovery cfg;
    in >> n >> dim >> cfg.warping_band_percentage >> cfg.insertion_penalty >> cfg.deletion_penalty >> cfg.match_penalty >>
        cfg.clustering_percentile;
    std::vector<apd::NDSequence> seqs(n);
    for (auto &s : seqs) {
        std::size_t len;
        in >> len;
        s.n_bins = dim;
        s.frames.resize(len * dim);
        for (auto &v : s.frames) in >> v;
    }
    try {
        apd::Context ctx(0);
        if (argc >= 4) {
            cfg = apd::Discovery::from_toml(argv[3]);
            std::printf("toml %zu %zu %zu %zu %.9g %zu %zu %.9g %.9g %.9g %.9g %.9g %zu %.9g %zu %.9g %.9g\n", cfg.dft_win, cfg.dft_step, cfg.ceps_filter,
                        cfg.vat_moving, cfg.vat_percentile, cfg.vat_min_len, cfg.alignment_workers, cfg.clustering_percentile,
                        cfg.warping_band_percentage, cfg.insertion_penalty, cfg.deletion_penalty, cfg.match_penalty, cfg.auto_encoder,
                        cfg.learning_rate, cfg.epochs, cfg.epoch_drop, cfg.drop);
            const apd::AutoEncoder nn = apd::AutoEncoder::from_file(argv[2]);
            std::printf("latent %zu\n", nn.n_latent());
            for (auto &s : seqs) s = nn.encoded(ctx, s);
            std::printf("enc0");
            for (float v : seqs[0].frames) std::printf(" %.9g", v);
            std::printf("\n");
            const std::string copy = std::string(argv[2]) + ".copy";
            nn.save_file(copy);
            std::ifstream a(argv[2], std::ios::binary), b(copy, std::ios::binary);
            const std::string sa((std::istreambuf_iterator<char>(a)), std::istreambuf_iterator<char>()), sb((std::istreambuf_iterator<char>(b)), std::istreambuf_iterator<char>());
            std::printf("roundtrip %d\n", (int)(sa == sb && !sa.empty()));
        }
        apd::AlignmentWorkers workers(ctx, seqs);
        workers.align_all(cfg);
        std::printf("dist");
        for (float v : workers.result) std::printf(" %.9g", v);
        std::printf("\n");
        {   // the multi-device entry with the one device a test box has: same bits, one rank
            const std::vector<float> single = workers.result;
            const uint32_t seen = workers.align_all(cfg, std::vector<int>{0});
            std::printf("multi %u %d\n", seen, (int)(std::memcmp(single.data(), workers.result.data(), single.size() * sizeof(float)) == 0));
            workers.align_all(cfg, std::vector<int>{0});                                  // the handle is kept: second call, same bits
            std::printf("multi_again %d %s\n", (int)(std::memcmp(single.data(), workers.result.data(), single.size() * sizeof(float)) == 0),
                        std::strncmp(workers.collective(), "rccl", 4) == 0 ? "rccl" : workers.collective());
        }
        auto res = apd::AgglomerativeClustering::clustering(ctx, workers.result, n, cfg.clustering_percentile);
        {   // SURVEY.md section 8(b)'s two one-call entry points, straight through the C ABI: same bits as the mirror's calls
            std::vector<float> flat;
            std::vector<uint64_t> off(1, 0);
            for (const auto &s : seqs) { flat.insert(flat.end(), s.frames.begin(), s.frames.end()); off.push_back(off.back() + s.len()); }
            std::vector<float> out(n * n, -1.0f);
            const int rc1 = apd_dtw_all_pairs(flat.data(), off.data(), (uint32_t)n, (uint32_t)seqs[0].n_bins, cfg.warping_band_percentage,
                                              cfg.insertion_penalty, cfg.deletion_penalty, cfg.match_penalty, 1, out.data());
            std::vector<apd_cluster_op> ops(n);
            std::vector<uint32_t> roots(n);
            uint32_t n_ops = 0, n_roots = 0;
            const int rc2 = apd_upgma(workers.result.data(), (uint32_t)n, cfg.clustering_percentile, ops.data(), &n_ops, roots.data(), &n_roots);
            bool same_ops = rc2 == 0 && n_ops == res.first.size() && n_roots == res.second.size();
            for (uint32_t t = 0; same_ops && t < n_ops; ++t)
                same_ops = ops[t].merge_i == res.first[t].merge_i && ops[t].merge_j == res.first[t].merge_j && ops[t].into == res.first[t].into &&
                           std::memcmp(&ops[t].distance, &res.first[t].distance, sizeof(float)) == 0;
            std::printf("onecall %d %d\n", (int)(rc1 == 0 && std::memcmp(out.data(), workers.result.data(), out.size() * sizeof(float)) == 0), (int)same_ops);
        }
        for (const auto &o : res.first) std::printf("op %zu %zu %zu %.9g %d\n", o.merge_i, o.merge_j, o.into, o.distance, (int)o.operation);
        std::printf("roots");
        for (auto r : res.second) std::printf(" %zu", r);
        std::printf("\n");
        for (const auto &s : apd::AgglomerativeClustering::cluster_sets(res.first, res.second, n)) {
            std::printf("set");
            for (auto m : s) std::printf(" %zu", m);
            std::printf("\n");
        }
        std::vector<std::string> labels;
        for (std::size_t i = 0; i < n; ++i) labels.push_back("{img" + std::to_string(i) + "}");
        for (const auto &kv : apd::dendrograms(res.first, res.second, labels)) std::printf("dendro %zu %s\n", kv.first, kv.second.c_str());
        apd::Alignment a(ctx);
        a.construct_alignment(seqs[0], seqs[1], cfg.alignment_params(std::max(seqs[0].len(), seqs[1].len())));
        std::printf("pair01 %.9g\n", a.score());
    } catch (const apd::Error &e) {
        std::printf("error %d %s\n", e.status, e.what());
        return 1;
    }
    return 0;
}
