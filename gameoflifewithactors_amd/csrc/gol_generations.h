// gol_generations.h -- the Generations family (B.../S.../C<n>): a life-like rule plus n - 2 "dying" states a cell walks
// through before it is dead again (Brian's Brain B2/S/3, Star Wars B2/S345/4, Frogs B34/S12/3).  Its scalar definition,
// its text forms, its bit-plane encoding and the bit-sliced decay of 32 cells per word (host + gfx950 device).  No HIP
// here beyond gol_bitlogic.h's host/device marker: gol_batch.cpp uses it for gol_generations_parse /
// gol_generations_format, gol_batch_wave.h for the kernels, and tests/cpp/test_generations.cpp compiles it alone
// under the address and undefined-behaviour sanitizers.
//
// Definition.  A cell's state is s in 0 .. C - 1, C = nstates in 2..8: 0 dead, 1 alive, 2 .. C - 1 dying.  n = the number
// of its 8 neighbours in state 1.
//   s = 0  -> 1 if bit n of birth is set, else 0
//   s = 1  -> 1 if bit n of survive is set, else 2 (C > 2) or 0 (C = 2)
//   s >= 2 -> s + 1 if s + 1 < C, else 0
// C = 2 is exactly the life-like rule.
//
// Encoding.  One alive plane A (bit = the cell is in state 1) and P = gen_planes(C) decay planes D_0 .. D_{P-1} that hold
// d = s - 1 of a dying cell as a binary number, bit k in D_k; a dead or alive cell has d = 0.  d runs 1 .. C - 2, so
// P = 0, 1, 2, 3 for C = 2, 3, 4..5, 6..8.  A and every D_k are exclusive: A & D_k = 0.  Pad bits (cells at or beyond W
// in a row's last word) are zero in every plane.
//
// Transition of one word (gen_decay), given v = the life-like rule's next state of the alive plane (rule_next_row: born
// where A = 0, surviving where A = 1; only state-1 cells are neighbours, so its sums are the alive plane's):
//   dying = OR D_k             A' = v & ~dying                 (births go to state-0 cells only)
//   died  = A & ~v             (d = 0 there)
//   keep  = dying & (d != C - 2)                                (a cell at the last dying state goes to 0)
//   D'    = keep ? d + 1 : died ? 1 : 0
// C - 2 enters as P scalar masks (bit k of C - 2 spread over a word: gen_masks), so nstates is a run-time value.
// Invariants: a pad bit is zero in A (cut by the caller's lastmask before v gets here or zero in v), so died, dying and
// keep are zero there and every D'_k keeps it zero; no bit of one cell reaches another, so what a lane holds that is no
// row of the board stays in that lane.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "gol_bitlogic.h"
#include "gol_rule.h"

namespace gol {

constexpr int kGenStatesMin = 2, kGenStatesMax = 8;
constexpr int kGenPlanesMax = 3;
constexpr int kGenFormatLen = 25;  // "B012345678/S012345678/C8" and its NUL

inline bool gen_states_ok(int nstates) { return nstates >= kGenStatesMin && nstates <= kGenStatesMax; }
constexpr int gen_planes(int nstates) { return nstates <= 2 ? 0 : nstates == 3 ? 1 : nstates <= 5 ? 2 : 3; }

// The definition: the next state of a cell in state s with n (0..8) neighbours in state 1.
GOL_HD int gen_next_cell(int s, int n, int birth, int survive, int nstates) {
    if (s == 0) return birth >> n & 1;
    if (s == 1) return (survive >> n & 1) ? 1 : nstates > 2 ? 2 : 0;
    return s + 1 < nstates ? s + 1 : 0;
}

// Bit k of C - 2 spread over a word.
struct GenMasks {
    uint32_t m[kGenPlanesMax];
};
GOL_HD GenMasks gen_masks(int nstates) {
    GenMasks g;
    for (int k = 0; k < kGenPlanesMax; k++) g.m[k] = ((nstates - 2) >> k & 1) ? 0xffffffffu : 0u;
    return g;
}

// 32 cells: `alive` = A before the generation, `v` = the life-like rule's next state of A, d = the decay planes (in
// place).  Returns A'.  P >= 1 (a 2-state board has no decay and never comes here).
template <int P>
GOL_HD uint32_t gen_decay(uint32_t alive, uint32_t v, uint32_t (&d)[P], const GenMasks& g) {
    static_assert(P >= 1 && P <= kGenPlanesMax, "1..3 decay planes");
    uint32_t dying = d[0], differs = d[0] ^ g.m[0];
    for (int k = 1; k < P; k++) {
        dying |= d[k];
        differs |= d[k] ^ g.m[k];
    }
    const uint32_t died = alive & ~v;
    const uint32_t keep = dying & differs;
    uint32_t carry = keep;  // d + 1 under keep
    for (int k = 0; k < P; k++) {
        const uint32_t bit = d[k];
        d[k] = (bit ^ carry) & keep;
        carry &= bit;
    }
    d[0] |= died;
    return v & ~dying;
}

// The indicator word of state k (1 .. C - 1) from a cell word's planes; k = 1 is the alive plane.  d = k - 1 >= 1 names
// at least one plane uninverted, so pad bits stay zero.
template <class Plane>
GOL_HD uint32_t gen_state_word(uint32_t alive, Plane&& plane, int planes, int k) {
    if (k == 1) return alive;
    uint32_t r = 0xffffffffu;
    for (int q = 0; q < planes; q++) r &= ((k - 1) >> q & 1) ? plane(q) : ~plane(q);
    return r;
}

// One cell between its state byte s (0 .. C - 1) and the encoding above: the alive bit and d = s - 1 of a dying cell
// (0 for a dead or alive one).  to_state = false: s -> (alive, d); true: (alive, d) -> s.  The state I/O kernels of the
// batch's planes aside, every conversion of a board handle goes through here (gol_formats.hip).
GOL_HD void gen_cell_convert(bool to_state, int& s, uint32_t& alive, uint32_t& d) {
    if (to_state) {
        s = alive ? 1 : d ? (int)d + 1 : 0;
    } else {
        alive = s == 1 ? 1u : 0u;
        d = s >= 2 ? (uint32_t)(s - 1) : 0u;
    }
}

// "<rule>" or "<rule>/<n>", "<rule>/C<n>", "<rule>/G<n>" (any letter case), <rule> everything rule_parse accepts, n one
// digit 2..8; blanks (space, tab) around the whole text only.  No third field: nstates 2.  Returns true and sets all
// three, or false with *why set and all three untouched.
inline bool generations_parse(const char* text, int* birth, int* survive, int* nstates, const char** why) {
    const auto no = [&](const char* w) {
        if (why) *why = w;
        return false;
    };
    if (!birth || !survive || !nstates) return no("null output");
    if (!text) return no("null rule text");
    int len = 0;
    while (len <= kRuleTextMax && text[len]) len++;
    if (len > kRuleTextMax) return no("rule text longer than 31 characters");
    int lo = 0, hi = len;
    while (lo < hi && (text[lo] == ' ' || text[lo] == '\t')) lo++;
    while (hi > lo && (text[hi - 1] == ' ' || text[hi - 1] == '\t')) hi--;
    int slashes = 0, second = -1;
    for (int i = lo; i < hi; i++)
        if (text[i] == '/' && ++slashes == 2) second = i;
    if (slashes > 2) return no("a Generations rule has at most three fields");
    int b = 0, s = 0, n = 2;
    if (slashes == 2) {
        int i = second + 1;
        if (i < hi && (text[i] == 'C' || text[i] == 'c' || text[i] == 'G' || text[i] == 'g')) i++;
        if (i + 1 != hi || text[i] < '2' || text[i] > '8')
            return no("the third field is <n>, C<n> or G<n> with n one digit 2..8");
        n = text[i] - '0';
        if (second > lo && (text[second - 1] == ' ' || text[second - 1] == '\t'))
            return no("a rule is B<digits>/S<digits>, S<digits>/B<digits> or <digits>/<digits>");
        char two[kRuleTextMax + 1];
        for (int k = lo; k < second; k++) two[k - lo] = text[k];
        two[second - lo] = 0;
        if (!rule_parse(two, &b, &s, why)) return false;
    } else if (!rule_parse(text, &b, &s, why)) {
        return false;
    }
    *birth = b;
    *survive = s;
    *nstates = n;
    return true;
}

// rule_format's text, and "/C<n>" behind it for n > 2, with its NUL into out[len]; len >= kGenFormatLen whatever n.
// A refusal writes nothing.
inline bool generations_format(int birth, int survive, int nstates, char* out, int64_t len, const char** why) {
    if (!rule_masks_ok(birth, survive)) {
        if (why) *why = "birth and survive masks must lie in 0..0x1FF";
        return false;
    }
    if (!gen_states_ok(nstates)) {
        if (why) *why = "nstates must be 2..8";
        return false;
    }
    if (!out || len < kGenFormatLen) {
        if (why) *why = "the rule's text needs a buffer of 25 characters";
        return false;
    }
    if (!rule_format(birth, survive, out, len, why)) return false;
    if (nstates > 2) {
        int k = 0;
        while (out[k]) k++;
        out[k++] = '/';
        out[k++] = 'C';
        out[k++] = (char)('0' + nstates);
        out[k] = 0;
    }
    return true;
}

}  // namespace gol
