// gol_seed_rle.h -- the host-only parts of seeding: the .NET System.Random restatement behind gol_seed_dotnet and the
// Life RLE parser behind gol_place_rle.  No HIP header: tests/cpp/test_seed_rle.cpp compiles it alone for the host.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

namespace gol {

// ---------------------------------------------------------------- .NET Framework System.Random
// Product restatement used by gol_seed_dotnet (GameOfLifeDriver.fs:10-11, GameofLife.fs:141-142,
// Script.fsx:25,27): Knuth subtractive generator, MSEED 161803398, 56-entry table, inext/inextp 0/21.
class DotNetRandom {
   public:
    explicit DotNetRandom(int32_t seed) {
        const int32_t mbig = 2147483647;
        int32_t sub = (seed == INT32_MIN) ? mbig : std::abs(seed);
        int32_t mj = 161803398 - sub, mk = 1;
        table_[55] = mj;
        for (int i = 1; i < 55; i++) {
            int ii = (21 * i) % 55;
            table_[ii] = mk;
            mk = (int32_t)((uint32_t)mj - (uint32_t)mk);
            if (mk < 0) mk += mbig;
            mj = table_[ii];
        }
        for (int k = 1; k < 5; k++)
            for (int i = 1; i < 56; i++) {
                table_[i] = (int32_t)((uint32_t)table_[i] - (uint32_t)table_[1 + (i + 30) % 55]);
                if (table_[i] < 0) table_[i] += mbig;
            }
    }
    int32_t Next() { return sample(); }
    int32_t Next(int32_t max_value) { return (int32_t)(sample() * (1.0 / 2147483647) * max_value); }

   private:
    int32_t sample() {
        if (++inext_ >= 56) inext_ = 1;
        if (++inextp_ >= 56) inextp_ = 1;
        int32_t r = (int32_t)((uint32_t)table_[inext_] - (uint32_t)table_[inextp_]);
        if (r == 2147483647) r--;
        if (r < 0) r += 2147483647;
        table_[inext_] = r;
        return r;
    }
    int32_t table_[56] = {0};
    int inext_ = 0, inextp_ = 21;
};

// ---------------------------------------------------------------- RLE (Life run-length encoding)
inline bool parse_rle(const char* p, std::vector<std::pair<int64_t, int64_t>>& out, std::string& err) {
    if (!p) {
        err = "null RLE";
        return false;
    }
    // skip '#' comment lines and the "x = .., y = .." header line
    for (;;) {
        while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') p++;
        if (*p == '#' || *p == 'x') {
            while (*p && *p != '\n') p++;
            continue;
        }
        break;
    }
    int64_t dx = 0, dy = 0, count = 0;
    for (; *p && *p != '!'; p++) {
        const char c = *p;
        if (c >= '0' && c <= '9') {
            count = count * 10 + (c - '0');
            if (count > (int64_t)1 << 40) {
                err = "RLE run length too large";
                return false;
            }
            continue;
        }
        if (c == ' ' || c == '\t' || c == '\r' || c == '\n') continue;
        const int64_t n = count ? count : 1;
        count = 0;
        if (c == '$') {
            dy += n;
            dx = 0;
        } else if (c == 'b' || c == '.') {
            dx += n;
        } else if ((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z')) {
            for (int64_t i = 0; i < n; i++) out.emplace_back(dx + i, dy);
            dx += n;
        } else {
            err = std::string("bad RLE character '") + c + "'";
            return false;
        }
    }
    return true;
}

}  // namespace gol
