// ssim_plan_test -- the host side of nsk_image_ssim (csrc/nsk_ssim_plan.h) alone, under the sanitizers (tests/test_ssim_plan_cpu.py): the
// window, the level sizes and the smallest side that holds them, the combine on known sums, on empty levels and at the array bounds.
#include <cmath>
#include <cstdio>
#include <vector>

#include "nsk_ssim_plan.h"

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

int main()
{
    // the window: symmetric, positive, sums to 1 within a rounding per tap, for every allowed size
    for (int win = 3; win <= SSIM_MAX_WIN; win += 2) {
        std::vector<double> g(win);             // exactly win entries: a write past the end is the sanitizer's to find
        ssim_window(win, 1.5, g.data());
        double s = 0.0;
        for (int k = 0; k < win; ++k) { s += g[k]; EXPECT(g[k] > 0.0 && g[k] == g[win - 1 - k]); }
        EXPECT(std::fabs(s - 1.0) < 1e-15 * win && g[win / 2] > g[0]);
    }
    // the sizes: 161 x 176 -> 81 x 88 -> 41 x 44 -> 21 x 22 -> 11 x 11
    {
        int H[5], W[5];
        EXPECT(ssim_plan_levels(161, 176, 11, 5, H, W) == -1);
        const int wantH[5] = {161, 81, 41, 21, 11}, wantW[5] = {176, 88, 44, 22, 11};
        for (int l = 0; l < 5; ++l) EXPECT(H[l] == wantH[l] && W[l] == wantW[l]);
        EXPECT(ssim_plan_levels(160, 176, 11, 5, H, W) == 4 && H[4] == 10);
        EXPECT(ssim_min_side(11, 5) == 161 && ssim_min_side(11, 1) == 11 && ssim_min_side(7, 3) == 25);
    }
    // the smallest side is the smallest: for every window and depth, it passes and one less fails
    for (int win = 3; win <= SSIM_MAX_WIN; win += 2)
        for (int levels = 1; levels <= SSIM_MAX_LEVELS; ++levels) {
            std::vector<int> H(levels), W(levels);
            const int m = (int)ssim_min_side(win, levels);
            EXPECT(ssim_plan_levels(m, m, win, levels, H.data(), W.data()) == -1 && H[levels - 1] == win);
            EXPECT(ssim_plan_levels(m - 1, m, win, levels, H.data(), W.data()) == levels - 1);
            EXPECT(ssim_plan_levels(m, m - 1, win, levels, H.data(), W.data()) == levels - 1);
        }
    // the combine at its largest: 8 levels, 4 channels
    {
        const int L = SSIM_MAX_LEVELS, C = SSIM_MAX_C;
        std::vector<double> sums((size_t)L * C * 3), w(L, 1.0 / L), h((size_t)L * C * 4);
        for (int l = 0; l < L; ++l) for (int c = 0; c < C; ++c) { double* s = &sums[((size_t)l * C + c) * 3]; s[0] = 5.0; s[1] = 2.5; s[2] = 10.0; }
        double out[2];
        ssim_combine(L, C, sums.data(), w.data(), h.data(), out);
        const double want = std::pow(0.25, 7.0 / 8.0) * std::pow(0.5, 1.0 / 8.0);
        EXPECT(std::fabs(out[0] - want) < 1e-14 && out[1] == 0.5);
        EXPECT(h[3] == 0.25 && h[((size_t)(L - 1) * C + C - 1) * 4 + 3] == 0.5 && h[2] == 10.0);
        // a negative mean counts as 0; an empty channel-level makes the result NaN and is no error
        sums[1] = -1.0;
        ssim_combine(L, C, sums.data(), w.data(), nullptr, out);
        EXPECT(std::fabs(out[0] - 0.75 * want) < 1e-14);
        sums[1] = 2.5; sums[((size_t)3 * C + 2) * 3 + 2] = 0.0;
        ssim_combine(L, C, sums.data(), w.data(), h.data(), out);
        EXPECT(out[0] != out[0] && out[1] == 0.5 && h[((size_t)3 * C + 2) * 4 + 3] != h[((size_t)3 * C + 2) * 4 + 3]);
    }
    // one level: the result is the level-0 SSIM, the weights are not read
    {
        const double sums[6] = {3.0, 1.0, 4.0, 1.0, 1.0, 4.0};
        double out[2], h[8];
        ssim_combine(1, 2, sums, nullptr, h, out);
        EXPECT(out[0] == 0.5 && out[1] == 0.5 && h[3] == 0.75 && h[7] == 0.25);
    }
    const double* sw = ssim_standard_weights();
    EXPECT(std::fabs(((((sw[0] + sw[1]) + sw[2]) + sw[3]) + sw[4]) - 1.0001) < 1e-12);
    if (failures == 0) std::printf("ssim_plan_test: ok\n");
    return failures == 0 ? 0 : 1;
}
