// The index tables of the decoder images (csrc/nsk_images.h) on the CPU: no torch, no HIP.  tests/test_images_cpu.py runs it.
//   images_test [table]   builds every table and every inverse of decoders 0..3, checks the properties below, prints one line per table
//                         `which what length set covered fnv` (set: entries >= 0; covered: distinct parameters; fnv: FNV-1a 64 over the entries
//                         as little-endian int32) and, given a recorded table (tests/golden/decoder_image_tables.txt), compares the lines with it
// Exit status 0: every property holds and every line is the recorded one.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "nsk_images.h"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t fnv1a(const std::vector<int>& v)
{
    uint64_t h = 1469598103934665603ull;
    for (int x : v) for (int b = 0; b < 4; ++b) { h ^= ((uint32_t)x >> (8 * b)) & 0xffu; h *= 1099511628211ull; }
    return h;
}

int main(int argc, char** argv)
{
    std::vector<std::string> lines;
    for (int which = 0; which < 4; ++which) {
        const int total = nsk_dec_layout(which).total;
        const size_t n4 = ((size_t)total + 3) & ~(size_t)3;
        std::vector<int> idx[NSK_NUM_IMAGES], inv[NSK_NUM_IMAGES];
        int set[NSK_NUM_IMAGES] = {0, 0, 0, 0};
        for (int what = 0; what < NSK_NUM_IMAGES; ++what) {
            build_image_table(which, what, idx[what]);
            const std::vector<int>& t = idx[what];
            for (int pieces = 2; pieces <= 3; ++pieces) {
                const ImageSpec s = image_spec(which, what, pieces);
                EXPECT(s.entries == (int)t.size(), "decoder %d image %d: the spec has %d entries, the table %zu", which, what, s.entries, t.size());
                EXPECT(s.floats == (s.pieces ? s.tail_off + s.tail_n : s.entries) && (what < 2 || which == 0 || s.pieces == (what == 2 ? pieces : 2)),
                       "decoder %d image %d: the spec's sizes", which, what);
            }
            if (t.empty()) { EXPECT(which == 0 && what >= 2, "decoder %d image %d is empty", which, what); continue; }
            bool in_range = true;
            for (int k : t) { if (k < -1 || k >= total) in_range = false; else if (k >= 0) ++set[what]; }
            EXPECT(in_range, "decoder %d image %d: an entry outside [-1, %d)", which, what, total);
            if (!in_range) continue;
            const int twice = invert_table(t, n4, inv[what]);
            EXPECT(twice == -1, "decoder %d image %d: parameter %d appears twice", which, what, twice);
            int covered = 0, back = 0;
            for (size_t k = 0; k < n4; ++k) if (inv[what][k] >= 0) { ++covered; if (t[inv[what][k]] == (int)k) ++back; }
            bool forth = twice == -1;
            for (size_t e = 0; forth && e < t.size(); ++e) if (t[e] >= 0 && inv[what][t[e]] != (int)e) forth = false;
            EXPECT(forth && back == covered, "decoder %d image %d: the inverse does not invert", which, what);
            EXPECT(twice != -1 || covered == set[what], "decoder %d image %d: %d set, %d covered", which, what, set[what], covered);
            if (what == 0) EXPECT(covered == total, "decoder %d: the fp32 forward image covers %d of %d parameters", which, covered, total);
            char buf[128];
            snprintf(buf, sizeof(buf), "%d %d %zu %d %d %016llx", which, what, t.size(), set[what], covered, (unsigned long long)fnv1a(t));
            lines.push_back(buf);
        }
        // the fp32 tail of an image in pieces: the end of the sibling's table, parameters its own fragments do not hold; fragments and tail
        // together hold what the sibling holds
        for (int what = 2; what < NSK_NUM_IMAGES && which != 0; ++what) {
            const ImageSpec s = image_spec(which, what, 2);
            const std::vector<int>& sib = idx[what - 2];
            EXPECT(s.tail_n > 0 && s.sib_off >= 0 && (size_t)s.sib_off + s.tail_n == sib.size(), "decoder %d image %d: the tail is not the end of image %d", which, what, what - 2);
            if ((size_t)s.sib_off + s.tail_n != sib.size() || inv[what].size() != n4) continue;
            int tail_set = 0;
            for (int e = s.sib_off; e < s.sib_off + s.tail_n; ++e) {
                const int k = sib[e];
                EXPECT(k >= -1 && k < total, "decoder %d image %d: tail entry %d out of range", which, what, e);
                if (k < 0 || k >= total) continue;
                ++tail_set;
                EXPECT(inv[what][k] == -1, "decoder %d image %d: parameter %d is in the fragments and in the tail", which, what, k);
            }
            EXPECT(set[what] + tail_set == set[what - 2], "decoder %d image %d: fragments %d + tail %d parameters, image %d has %d", which, what, set[what], tail_set, what - 2, set[what - 2]);
        }
    }
    for (const std::string& l : lines) printf("%s\n", l.c_str());
    if (argc > 1) {
        FILE* f = fopen(argv[1], "r");
        if (!f) { printf("images_test: cannot open %s\n", argv[1]); return 2; }
        std::vector<std::string> want;
        char buf[256];
        while (fgets(buf, sizeof(buf), f)) {
            std::string l(buf);
            while (!l.empty() && (l.back() == '\n' || l.back() == '\r' || l.back() == ' ')) l.pop_back();
            if (!l.empty() && l[0] != '#') want.push_back(l);
        }
        fclose(f);
        EXPECT(want.size() == lines.size(), "%zu tables, %zu recorded", lines.size(), want.size());
        for (size_t i = 0; i < lines.size() && i < want.size(); ++i) EXPECT(lines[i] == want[i], "table `%s`, recorded `%s`", lines[i].c_str(), want[i].c_str());
    }
    printf("images_test: %zu tables, %d failures\n", lines.size(), failures);
    return failures ? 1 : 0;
}
