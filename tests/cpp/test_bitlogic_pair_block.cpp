// Host check of the block forms of the row-pair rule (row_sum_block_staged / pair_sum_block / pair_g13_block /
// pair_g2_block / pair_next_block, gameoflifewithactors_amd/csrc/gol_bitlogic.h: the pipelined pass's LUTs taken stage
// by stage over a block's M words) against the word forms they restage (row_sum_block, pair_sum, life_next_pair),
// against life_next, and against the reference rule (GameOfLifeLogic.fs:59-63).
//   1. every filling of a 4-row x 3-column neighbourhood, its centre column in each of the block's 4 words at the
//      first, a middle and the last bit -- so the neighbourhood also straddles the block's two edges, where the west
//      and east words come from the funnel shifts on the neighbour blocks' words: rows 1 and 2 are the pair,
//      out(1) = pair + row 0 with row 1's centre, out(2) = pair + row 3 with row 2's centre;
//   2. full random words, densities 0.1 to 1.0, M = 4: every word of both outputs.
// Built and run by tests/test_bitlogic_pair_block_host.py (CPU).
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "../../gameoflifewithactors_amd/csrc/gol_bitlogic.h"

constexpr int M = 4;

static int rule(int a, int alive) { return (a > 3 || a < 2) ? 0 : (a == 3 ? 1 : alive); }

struct Row {
    uint32_t w[M] = {0, 0, 0, 0};
    uint32_t prev_last = 0, next_first = 0;  // the left block's word M - 1, the right block's word 0
};

// cell x of a block row: word x % M, bit x / M (gol_layout.h); x = -1 and x = 32 M lie in the neighbour blocks
static void set_cell(Row& r, int x) {
    if (x < 0)
        r.prev_last |= 1u << 31;
    else if (x >= 32 * M)
        r.next_first |= 1u;
    else
        r.w[x % M] |= 1u << (x / M);
}

// Both outputs of the pair (rows[1], rows[2]) by the block forms, in the pipelined pass's order; returns the words that
// differ from the word forms (life_next_pair on pair_sum on row_sum_block) or from life_next
static int pair_block(const Row (&rows)[4], uint32_t (&o0)[M], uint32_t (&o1)[M]) {
    int bad = 0;
    uint32_t s[4][M], c[4][M], sr[4][M], cr[4][M];
    for (int r = 0; r < 4; r++) {
        const uint32_t w0 = gol::align_right(rows[r].w[M - 1], rows[r].prev_last, 31);
        const uint32_t eN = gol::align_right(rows[r].next_first, rows[r].w[0], 1);
        gol::row_sum_block_staged<M>(rows[r].w, w0, eN, s[r], c[r]);
        gol::row_sum_block<M>(rows[r].w, rows[r].prev_last, rows[r].next_first, sr[r], cr[r]);
        for (int j = 0; j < M; j++) bad += s[r][j] != sr[r][j] || c[r][j] != cr[r][j];
    }
    uint32_t q0[M], q1[M], q2[M], g1[M], g2[M], g3[M];
    gol::pair_sum_block<M>(s[1], c[1], s[2], c[2], q0, q1, q2);
    gol::pair_g13_block<M>(q0, q1, q2, s[0], c[0], rows[1].w, g1, g3);
    gol::pair_g2_block<M>(q2, rows[1].w, g1, g2);
    gol::pair_next_block<M>(g1, g2, g3, o0);
    gol::pair_g13_block<M>(q0, q1, q2, s[3], c[3], rows[2].w, g1, g3);
    gol::pair_g2_block<M>(q2, rows[2].w, g1, g2);
    gol::pair_next_block<M>(g1, g2, g3, o1);
    for (int j = 0; j < M; j++) {
        uint32_t p0, p1, p2;
        gol::pair_sum(sr[1][j], cr[1][j], sr[2][j], cr[2][j], p0, p1, p2);
        bad += p0 != q0[j] || p1 != q1[j] || p2 != q2[j];
        bad += o0[j] != gol::life_next_pair(p0, p1, p2, sr[0][j], cr[0][j], rows[1].w[j]);
        bad += o1[j] != gol::life_next_pair(p0, p1, p2, sr[3][j], cr[3][j], rows[2].w[j]);
        bad += o0[j] != gol::life_next(sr[0][j], cr[0][j], sr[1][j], cr[1][j], sr[2][j], cr[2][j], rows[1].w[j]);
        bad += o1[j] != gol::life_next(sr[1][j], cr[1][j], sr[2][j], cr[2][j], sr[3][j], cr[3][j], rows[2].w[j]);
    }
    return bad;
}

static int exhaustive() {
    int bad = 0;
    for (int j = 0; j < M; j++)
        for (int b : {0, 15, 31})
            for (int n = 0; n < 4096; n++) {
                const int x = j + M * b;  // the centre column
                Row rows[4];
                int cells[4][3];
                for (int k = 0; k < 12; k++) {
                    cells[k / 3][k % 3] = (n >> k) & 1;
                    if (cells[k / 3][k % 3]) set_cell(rows[k / 3], x + k % 3 - 1);
                }
                uint32_t o[2][M];
                bad += pair_block(rows, o[0], o[1]);
                for (int i = 0; i < 2; i++) {
                    int a = -cells[1 + i][1];
                    for (int dy = 0; dy < 3; dy++)
                        for (int dx = 0; dx < 3; dx++) a += cells[i + dy][dx];
                    if ((int)((o[i][j] >> b) & 1) != rule(a, cells[1 + i][1])) bad++;
                }
            }
    return bad;
}

static uint32_t rand_word(int density_pct) {
    uint32_t v = 0;
    for (int b = 0; b < 32; b++) v |= (uint32_t)(rand() % 100 < density_pct) << b;
    return v;
}

static int random_words() {
    int bad = 0;
    for (int density : {10, 25, 40, 50, 75, 90, 100})
        for (int it = 0; it < 4000; it++) {
            Row rows[4];
            for (Row& r : rows) {
                for (int j = 0; j < M; j++) r.w[j] = rand_word(density);
                r.prev_last = rand_word(density);
                r.next_first = rand_word(density);
            }
            uint32_t o0[M], o1[M];
            bad += pair_block(rows, o0, o1);
        }
    return bad;
}

int main() {
    srand(20241021);
    const int e = exhaustive(), r = random_words();
    std::printf("{\"exhaustive_mismatches\": %d, \"random_mismatches\": %d, \"mismatches\": %d}\n", e, r, e + r);
    return e + r != 0;
}
