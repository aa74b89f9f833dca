// nsk_ssim_plan.h -- the host side of nsk_image_ssim (include/nsk.h states the rule): the window's weights, the sizes of the pyramid's
// levels, and the combination of the levels' sums into SSIM / MS-SSIM.  Nothing here needs HIP: nsk.hip includes it, and
// host/test/ssim_plan_test.cpp runs it alone under the sanitizers.
#pragma once
#include <cmath>
#include <limits>

#define SSIM_MAX_WIN 15
#define SSIM_MAX_LEVELS 8
#define SSIM_MAX_C 4

// g_k = exp(-(k - win / 2)^2 / (2 sigma^2)) divided by the sum of the g_k taken in index order, in double
inline void ssim_window(int win, double sigma, double* g)
{
    double sum = 0.0;
    for (int k = 0; k < win; ++k) {
        const double d = (double)(k - win / 2);
        g[k] = std::exp(-(d * d) / (2.0 * (sigma * sigma)));
        sum = sum + g[k];
    }
    for (int k = 0; k < win; ++k) g[k] = g[k] / sum;
}

// the standard five weights (Wang et al. 2003), as doubles
inline const double* ssim_standard_weights()
{
    static const double w[5] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    return w;
}

// level l + 1 of a side: the 2 x 2 average with p = size mod 2 of padding on both ends, (size + 2 p) / 2 = ceil(size / 2)
inline int ssim_next_side(int size) { return (size + 2 * (size % 2)) / 2; }

// the smallest side whose last of `levels` levels still holds one window: (win - 1) 2^(levels - 1) + 1
inline long long ssim_min_side(int win, int levels) { return ((long long)(win - 1) << (levels - 1)) + 1; }

// sides of every level; returns the first level smaller than win on a side, or -1 when every level holds a window
inline int ssim_plan_levels(int Hv, int Wv, int win, int levels, int* Hl, int* Wl)
{
    int bad = -1;
    for (int l = 0; l < levels; ++l) {
        Hl[l] = l == 0 ? Hv : ssim_next_side(Hl[l - 1]);
        Wl[l] = l == 0 ? Wv : ssim_next_side(Wl[l - 1]);
        if (bad < 0 && (Hl[l] < win || Wl[l] < win)) bad = l;
    }
    return bad;
}

// sums [levels][C][3] (sum of ssim, sum of cs, windows counted) -> h_levels [levels][C][4] (the three sums and the value the level
// contributes: its mean cs, for the last level its mean ssim; NaN without a window) and out[0] the result, out[1] the level-0 SSIM.
// The result: levels = 1 the level-0 SSIM; else the mean over channels of prod_l max(value_l, 0)^w_l (a NaN value stays NaN).
inline void ssim_combine(int levels, int C, const double* sums, const double* weights, double* h_levels, double* out)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double ms = 0.0, s0 = 0.0;
    for (int c = 0; c < C; ++c) {
        double prod = 1.0;
        for (int l = 0; l < levels; ++l) {
            const double* s = sums + ((size_t)l * C + c) * 3;
            const double value = s[2] > 0.0 ? (l == levels - 1 ? s[0] : s[1]) / s[2] : nan;
            if (h_levels) {
                double* h = h_levels + ((size_t)l * C + c) * 4;
                h[0] = s[0]; h[1] = s[1]; h[2] = s[2]; h[3] = value;
            }
            if (levels > 1) prod = prod * std::pow(value > 0.0 ? value : (value != value ? value : 0.0), weights[l]);
        }
        const double* s = sums + (size_t)c * 3;
        s0 = s0 + (s[2] > 0.0 ? s[0] / s[2] : nan);
        ms = ms + prod;
    }
    out[1] = s0 / (double)C;
    out[0] = levels > 1 ? ms / (double)C : out[1];
}
