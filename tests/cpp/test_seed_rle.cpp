// Host-only check of csrc/gol_seed_rle.h (the .NET System.Random restatement of gol_seed_dotnet and the RLE parser of
// gol_place_rle): prints what they produce, one JSON object per line, for tests/test_cpu_host.py to compare with the
// oracle's own restatements (oracle/gol_oracle.py DotNetRandom, parse_rle).  Built with -fsanitize=address,undefined.
#include <cstdio>

#include "../../gameoflifewithactors_amd/csrc/gol_seed_rle.h"

static void print_random(int32_t seed) {
    gol::DotNetRandom a(seed), b(seed);
    std::printf("{\"seed\": %d, \"next\": [", seed);
    for (int i = 0; i < 64; i++) std::printf("%s%d", i ? ", " : "", a.Next());
    std::printf("], \"next2\": [");
    for (int i = 0; i < 64; i++) std::printf("%s%d", i ? ", " : "", b.Next(2));
    std::printf("]}\n");
}

static void print_rle(const char* name, const char* rle) {
    std::vector<std::pair<int64_t, int64_t>> pts;
    std::string err;
    const bool ok = gol::parse_rle(rle, pts, err);
    std::printf("{\"rle\": \"%s\", \"ok\": %s, \"error\": \"%s\", \"points\": [", name, ok ? "true" : "false",
                err.c_str());
    if (ok)
        for (size_t i = 0; i < pts.size(); i++)
            std::printf("%s[%lld, %lld]", i ? ", " : "", (long long)pts[i].first, (long long)pts[i].second);
    std::printf("]}\n");
}

int main() {
    for (int32_t seed : {0, 1, 42, -5, INT32_MIN}) print_random(seed);
    // the same strings, under the same names, as RLE in tests/test_cpu_host.py
    print_rle("glider", "bo$2bo$3o!");
    print_rle("header", "#N Gosper glider gun\n#C a comment\nx = 36, y = 9, rule = B3/S23\n24bo$22bobo$12b2o6b2o12b2o$11bo3bo4b2o12b2o$\n2o8bo5bo3b2o$2o8bo3bob2o4bobo$10bo5bo7bo$11bo3bo$12b2o!");
    print_rle("long_runs", "12o13$\n15b10o2$ 3o.A!");
    print_rle("bad_character", "3o$2b?o!");
    print_rle("huge_run", "2o$1099511627777o!");
    print_rle("null", nullptr);
    return 0;
}
