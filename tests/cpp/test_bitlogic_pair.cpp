// Host check of the row-pair form of the rule (pair_sum / life_next_pair, gameoflifewithactors_amd/csrc/gol_bitlogic.h:
// 8 LUT ops per word and generation) against life_next, and life_next's own reference rule (GameOfLifeLogic.fs:59-63).
//   1. every filling of a 4-row x 3-column neighbourhood, at several bit positions of the centre word: rows 1 and 2 are
//      the pair, out(1) = pair + row 0 with row 1's centre, out(2) = pair + row 3 with row 2's centre;
//   2. full 32-bit random words on a small torus of interleaved 4-word blocks (row_sum_block<4>), stepped for a few
//      generations with the pipelined pass's window rotation (gol_pipe.hip), every row against life_next: an operand
//      order slip (which row is "the other", which word is the centre) shows here and not in a single column.
// Built and run by tests/test_bitlogic_pair_host.py (CPU).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "../../gameoflifewithactors_amd/csrc/gol_bitlogic.h"

static int rule(int a, int alive) { return (a > 3 || a < 2) ? 0 : (a == 3 ? 1 : alive); }

static int exhaustive() {
    int bad = 0;
    for (int p : {0, 1, 15, 30, 31})
        for (int n = 0; n < 4096; n++) {
            uint32_t rows[4][3] = {{0}};
            int cells[4][3];
            for (int k = 0; k < 12; k++) {
                const int dy = k / 3, dx = k % 3 - 1, x = p + dx;
                cells[dy][k % 3] = (n >> k) & 1;
                if (cells[dy][k % 3]) rows[dy][1 + (x < 0 ? -1 : (x >= 32 ? 1 : 0))] |= 1u << ((x + 32) & 31);
            }
            uint32_t s[4], c[4], q0, q1, q2;
            for (int r = 0; r < 4; r++) gol::row_sum(rows[r][0], rows[r][1], rows[r][2], s[r], c[r]);
            gol::pair_sum(s[1], c[1], s[2], c[2], q0, q1, q2);
            const uint32_t got[2] = {gol::life_next_pair(q0, q1, q2, s[0], c[0], rows[1][1]),
                                     gol::life_next_pair(q0, q1, q2, s[3], c[3], rows[2][1])};
            const uint32_t ref[2] = {gol::life_next(s[0], c[0], s[1], c[1], s[2], c[2], rows[1][1]),
                                     gol::life_next(s[1], c[1], s[2], c[2], s[3], c[3], rows[2][1])};
            for (int o = 0; o < 2; o++) {
                int a = -cells[1 + o][1];
                for (int dy = 0; dy < 3; dy++)
                    for (int dx = 0; dx < 3; dx++) a += cells[o + dy][dx];
                if ((int)((got[o] >> p) & 1) != rule(a, cells[1 + o][1])) bad++;
                if (got[o] != ref[o]) bad++;  // the bits of the other columns too (their neighbourhoods are partial ones)
            }
        }
    return bad;
}

// A torus of H rows x B blocks of 4 interleaved words
constexpr int M = 4, H = 10, B = 3;
typedef uint32_t Board[H][B][M];

static void sums(const Board& b, int y, int k, uint32_t (&s)[M], uint32_t (&c)[M]) {
    y = (y % H + H) % H;
    gol::row_sum_block<M>(b[y][k], b[y][(k + B - 1) % B][M - 1], b[y][(k + 1) % B][0], s, c);
}

static void step_ref(const Board& in, Board& out) {
    for (int y = 0; y < H; y++)
        for (int k = 0; k < B; k++) {
            uint32_t sP[M], cP[M], sC[M], cC[M], sN[M], cN[M];
            sums(in, y - 1, k, sP, cP);
            sums(in, y, k, sC, cC);
            sums(in, y + 1, k, sN, cN);
            for (int j = 0; j < M; j++) out[y][k][j] = gol::life_next(sP[j], cP[j], sC[j], cC[j], sN[j], cN[j], in[y][k][j]);
        }
}

// Rows enter in pairs (r, r + 1) and leave as outputs (r - 1, r), with the carried window X = row r - 2, Y = row r - 1
// and Y's centre word, rotated X <- N, Y <- N' as the pipelined pass does
static void step_pair(const Board& in, Board& out) {
    for (int k = 0; k < B; k++) {
        uint32_t sX[M], cX[M], sY[M], cY[M], aY[M];
        sums(in, -2, k, sX, cX);
        sums(in, -1, k, sY, cY);
        std::memcpy(aY, in[H - 1][k], sizeof aY);
        for (int r = 0; r < H; r += 2) {
            uint32_t sN[M], cN[M], sN1[M], cN1[M];
            sums(in, r, k, sN, cN);
            sums(in, r + 1, k, sN1, cN1);
            for (int j = 0; j < M; j++) {
                uint32_t q0, q1, q2;
                gol::pair_sum(sY[j], cY[j], sN[j], cN[j], q0, q1, q2);
                out[(r + H - 1) % H][k][j] = gol::life_next_pair(q0, q1, q2, sX[j], cX[j], aY[j]);
                out[r][k][j] = gol::life_next_pair(q0, q1, q2, sN1[j], cN1[j], in[r][k][j]);
                sX[j] = sN[j];
                cX[j] = cN[j];
                sY[j] = sN1[j];
                cY[j] = cN1[j];
                aY[j] = in[r + 1][k][j];
            }
        }
    }
}

static uint32_t rand_word(int density_pct) {
    uint32_t v = 0;
    for (int b = 0; b < 32; b++) v |= (uint32_t)(rand() % 100 < density_pct) << b;
    return v;
}

static int random_torus() {
    int bad = 0;
    static_assert(H % 2 == 0, "rows in pairs");
    for (int density : {10, 40, 50, 90, 100})
        for (int it = 0; it < 400; it++) {
            static Board a, ref, got;
            for (int y = 0; y < H; y++)
                for (int k = 0; k < B; k++)
                    for (int j = 0; j < M; j++) a[y][k][j] = rand_word(density);
            for (int gen = 0; gen < 4; gen++) {
                step_ref(a, ref);
                step_pair(a, got);
                for (int y = 0; y < H; y++)
                    for (int k = 0; k < B; k++)
                        for (int j = 0; j < M; j++) bad += got[y][k][j] != ref[y][k][j];
                std::memcpy(a, got, sizeof a);
            }
        }
    return bad;
}

int main() {
    srand(20240607);
    const int e = exhaustive(), r = random_torus();
    std::printf("{\"exhaustive_mismatches\": %d, \"torus_mismatches\": %d, \"mismatches\": %d}\n", e, r, e + r);
    return e + r != 0;
}
