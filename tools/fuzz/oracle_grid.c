/*
 * oracle_grid.c -- the CPU oracle's DTW (oracle/apd_oracle.c) walked over a grid of degenerate alignment configurations, built with
 * -fsanitize=address,undefined as a stand-alone program (tests/test_config_cases.py builds and runs it as a child process).
 *
 *   oracle_grid <grid file>
 *
 * Every line of the grid file is one configuration: three penalties (insertion, deletion, match) as the hex bits of their f32,
 * then `P <hex bits of the f32 percentage>` or `B <decimal u64 explicit band>`.  tests/_config_cases.py is the one table the lines
 * come from.  Every configuration runs over every ordered pair of a handful of tiny sequences (lengths 1, 2, 3, 7, 20, 33, both
 * orders and each against itself, so that |n-m| exceeds small bands): the dense form, the hash-map form and the cell count.  The
 * dense and the hash-map score must have the same bits (any NaN equals any NaN) and the cell count must lie in 1 .. n * m -- the
 * dense form writing outside its rows, or a window derived from a wrapped band, is what the sanitizer and these two comparisons
 * are there to see.  Prints one line per configuration (a checksum of the scores) and, at the end,
 * "no sanitizer report".
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "apd_oracle.h"

static const uint64_t kLengths[] = {1, 2, 3, 7, 20, 33};
enum { kNumLengths = 6, kDim = 3 };

static float f32_from_bits(uint32_t b) { float f; memcpy(&f, &b, sizeof(f)); return f; }
static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, sizeof(b)); return (f != f) ? 0x7FC00000u : b; }

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: oracle_grid <grid file>\n"); return 2; }
    FILE *fp = fopen(argv[1], "r");
    if (!fp) { perror(argv[1]); return 2; }
    /* the sequences: deterministic values on a grid of 1/32, the 3-frame one equal to the first frames of the 7-frame one (zero distances) */
    float *seq[kNumLengths];
    uint32_t state = 12345u;
    for (int s = 0; s < kNumLengths; s++) {
        seq[s] = (float *)malloc(sizeof(float) * kLengths[s] * kDim);     /* exact size: an overread is a sanitizer report */
        for (uint64_t k = 0; k < kLengths[s] * kDim; k++) {
            state = state * 1664525u + 1013904223u;
            seq[s][k] = (float)((int)(state >> 24) - 128) / 32.0f;
        }
    }
    memcpy(seq[2], seq[3], sizeof(float) * kLengths[2] * kDim);
    uint32_t ib, db, mb;
    char kind;
    char value[64];
    uint64_t runs = 0, configs = 0;
    int bad = 0;
    while (fscanf(fp, "%" SCNx32 " %" SCNx32 " %" SCNx32 " %c %63s", &ib, &db, &mb, &kind, value) == 5) {
        const float ins = f32_from_bits(ib), del = f32_from_bits(db), mat = f32_from_bits(mb);
        uint32_t sum = 0;
        for (int a = 0; a < kNumLengths; a++)
            for (int b = 0; b < kNumLengths; b++) {
                const uint64_t n = kLengths[a], m = kLengths[b], mx = n > m ? n : m;
                uint64_t band;
                if (kind == 'P') band = orc_warping_band(f32_from_bits((uint32_t)strtoul(value, NULL, 16)), mx);
                else if (kind == 'B') band = strtoull(value, NULL, 10);
                else { fprintf(stderr, "bad kind %c\n", kind); return 2; }
                const float dense = orc_dtw_pair(seq[a], n, seq[b], m, kDim, band, ins, del, mat);
                const float sparse = orc_dtw_pair_hashmap(seq[a], n, seq[b], m, kDim, band, ins, del, mat);
                const uint64_t cells = orc_dtw_cells(n, m, band);
                if (bits_of(dense) != bits_of(sparse)) {
                    printf("MISMATCH config %" PRIu64 " pair (%" PRIu64 ", %" PRIu64 "): dense %08x, hash map %08x\n", configs, n, m,
                           bits_of(dense), bits_of(sparse));
                    bad = 1;
                }
                if (cells == 0 || cells > n * m) {
                    printf("CELLS config %" PRIu64 " pair (%" PRIu64 ", %" PRIu64 "): %" PRIu64 " cells\n", configs, n, m, cells);
                    bad = 1;
                }
                sum = sum * 31u + bits_of(dense);
                runs++;
            }
        printf("config %" PRIu64 ": %08x\n", configs, sum);
        configs++;
    }
    fclose(fp);
    for (int s = 0; s < kNumLengths; s++) free(seq[s]);
    if (bad || configs == 0) return 1;
    printf("%" PRIu64 " configurations, %" PRIu64 " runs, no sanitizer report\n", configs, runs);
    return 0;
}
