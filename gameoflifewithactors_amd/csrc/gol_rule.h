// gol_rule.h -- a life-like rule (B.../S...) as two 9-bit masks: its text forms, its ranges and its scalar definition.
// No HIP here: gol_batch.cpp uses it for gol_rule_parse / gol_rule_format / gol_ensemble_set_rule, and
// tests/cpp/test_rule.cpp compiles it alone under the address and undefined-behaviour sanitizers, where it is also the
// definition the bit-sliced evaluator (gol_bitlogic.h rule_next) is checked against.
//
// Bit n (0..8) of `birth`: a dead cell with n live cells among its 8 neighbours becomes alive; bit n of `survive`: a
// live cell with n live neighbours stays alive.  Conway's rule is birth 0x008, survive 0x00C.  The kernels take both
// masks in one word, birth | survive << 9 (rule_pack).
#pragma once
#include <stdint.h>

namespace gol {

constexpr int kRuleMaskMax = 0x1FF;
constexpr int kRuleLifeBirth = 0x008, kRuleLifeSurvive = 0x00C;
constexpr int kRuleTextMax = 31;     // characters of a rule's text, blanks included
constexpr int kRuleFormatLen = 22;   // "B012345678/S012345678" and its NUL

inline bool rule_masks_ok(int birth, int survive) {
    return birth >= 0 && birth <= kRuleMaskMax && survive >= 0 && survive <= kRuleMaskMax;
}
inline uint32_t rule_pack(int birth, int survive) { return (uint32_t)birth | (uint32_t)survive << 9; }
constexpr uint32_t kRuleLifePacked = (uint32_t)kRuleLifeBirth | (uint32_t)kRuleLifeSurvive << 9;
inline bool rule_packed_ok(uint32_t packed) { return packed < (1u << 18); }

// Which kernels a launch runs.  Life: B3/S23 by life_next, the code every pass had before rules existed.  Table: any
// life-like rule by its packed masks -- every rule but B3/S23, and B3/S23 too under force_table (the "rule_table"
// options).  PerBoard: a batch with a table of one packed rule per board (`rules`), whatever `rule` and force_table
// say.
enum class RuleFamily { Life, Table, PerBoard };
inline RuleFamily rule_family(uint32_t rule, bool force_table, const uint32_t* rules = nullptr) {
    if (rules) return RuleFamily::PerBoard;
    return force_table || rule != kRuleLifePacked ? RuleFamily::Table : RuleFamily::Life;
}

// The definition: the next state of a cell with n (0..8) live neighbours among its 8.
inline int rule_next_cell(int alive, int n, int birth, int survive) {
    return alive ? survive >> n & 1 : birth >> n & 1;
}

// "B<digits>/S<digits>", "S<digits>/B<digits>" or "<survive digits>/<birth digits>", any letter case, blanks (space,
// tab) around it; digits 0..8, each at most once per list, in any order; either list may be empty.  Returns true and
// sets both masks, or returns false with *why set and both masks untouched.
inline bool rule_parse(const char* text, int* birth, int* survive, const char** why) {
    const auto no = [&](const char* w) {
        if (why) *why = w;
        return false;
    };
    if (!birth || !survive) return no("null output");
    if (!text) return no("null rule text");
    int len = 0;
    while (len <= kRuleTextMax && text[len]) len++;
    if (len > kRuleTextMax) return no("rule text longer than 31 characters");
    int lo = 0, hi = len;
    while (lo < hi && (text[lo] == ' ' || text[lo] == '\t')) lo++;
    while (hi > lo && (text[hi - 1] == ' ' || text[hi - 1] == '\t')) hi--;
    if (lo == hi) return no("empty rule text");
    int mask[2] = {0, 0};  // [0] birth, [1] survive
    int kind[2] = {-1, -1};  // what each half turned out to be: 0 birth, 1 survive, 2 digits only
    int half = 0;
    bool at_start = true;  // of the current half: a letter may stand here only
    int cur = 0;           // the mask the current half's digits go to
    for (int i = lo; i < hi; i++) {
        const char ch = text[i];
        if (ch == '/') {
            if (half == 1) return no("a rule has two fields (a third is the Generations family: not supported)");
            if (at_start) kind[0] = 2, cur = 1;  // an empty digits-only first half: survive
            half = 1;
            at_start = true;
            continue;
        }
        if (at_start) {
            at_start = false;
            const int k = (ch == 'B' || ch == 'b') ? 0 : (ch == 'S' || ch == 's') ? 1 : 2;
            kind[half] = k;
            cur = k == 2 ? (half == 0 ? 1 : 0) : k;  // digits only: survive first, then birth
            if (k != 2) continue;
        }
        if (ch < '0' || ch > '9') return no("a rule is B<digits>/S<digits>, S<digits>/B<digits> or <digits>/<digits>");
        if (ch == '9') return no("a cell has 8 neighbours: digits are 0..8");
        const int bit = 1 << (ch - '0');
        if (mask[cur] & bit) return no("a digit appears twice in one list");
        mask[cur] |= bit;
    }
    if (half == 0) return no("a rule needs a slash between its two fields");
    if (at_start) kind[1] = 2;  // an empty second half
    // both halves lettered (one B, one S), or neither
    const bool lettered = kind[0] != 2 && kind[1] != 2 && kind[0] != kind[1];
    const bool plain = kind[0] == 2 && kind[1] == 2;
    if (!lettered && !plain) return no("a rule names B and S once each, or neither");
    *birth = mask[0];
    *survive = mask[1];
    return true;
}

// The canonical form "B<ascending digits>/S<ascending digits>" and its NUL into out[len]; len >= kRuleFormatLen.
inline bool rule_format(int birth, int survive, char* out, int64_t len, const char** why) {
    if (!rule_masks_ok(birth, survive)) {
        if (why) *why = "birth and survive masks must lie in 0..0x1FF";
        return false;
    }
    if (!out || len < kRuleFormatLen) {
        if (why) *why = "the rule's text needs a buffer of 22 characters";
        return false;
    }
    int k = 0;
    out[k++] = 'B';
    for (int n = 0; n <= 8; n++)
        if (birth >> n & 1) out[k++] = (char)('0' + n);
    out[k++] = '/';
    out[k++] = 'S';
    for (int n = 0; n <= 8; n++)
        if (survive >> n & 1) out[k++] = (char)('0' + n);
    out[k] = 0;
    return true;
}

}  // namespace gol
