// nsk_split.h -- how a decoder launch divides its workgroups over its roles: cost model and split arithmetic in host integers, nothing of HIP
// (host/test/split_test.cpp builds it with a plain host compiler: tests/test_split_cpu.py)
#pragma once
#include <algorithm>

struct SplitTune {                          // nsk_set_tuning keys of the same names
    int fwd_occ_cost = 0;                   // the merged middle + fine role of the forward: its cost against the colour role's (0 = 460)
    int fwd_fine_cost = 0, fwd_color_cost = 0;     // experiments: forward role costs
    int frozen_cost = 0;                    // > 0: overrides the frozen-role cost of the backward's workgroup split (experiments)
    int frozen_cost_rays = 0;               // > 0: the same for launches with ray gradients (bundle adjustment: the frozen roles also carry g_e and d/dp)
    int frozen_mid_pct = 100;               // the middle decoder's frozen tile against the fine one's, in percent (its level has 8x the samples per voxel: more same-line atomics)
    int dead_tile_pct = 12;                 // what a skipped tile costs in the workgroup split, in percent of a tile that runs (its staged loads and the loop)
};

// forward: issue cycles per tile of the roles (coarse fp32; middle 7 560, fine 9 380, colour 7 710 + its block-output stores)
static inline int fwd_role_cost(int w, const SplitTune& t)
{
    static const int fcost[4] = {96, 240, 292, 248};
    return (w == 2 && t.fwd_fine_cost > 0) ? t.fwd_fine_cost : ((w == 3 && t.fwd_color_cost > 0) ? t.fwd_color_cost : fcost[w]);
}
static inline int fwd_occ_role_cost(const SplitTune& t) { return t.fwd_occ_cost > 0 ? t.fwd_occ_cost : 460; }
// backward: relative cost of one tile of a frozen role against one 8-tile iteration of the trainable role (= 1000)
static inline int bwd_role_cost(bool train, int w, bool rays, const SplitTune& t)
{
    const int frozen_cost = rays ? (t.frozen_cost_rays > 0 ? t.frozen_cost_rays : 330) : (t.frozen_cost > 0 ? t.frozen_cost : 205);
    return train ? 1000 : (w == 1 ? frozen_cost * t.frozen_mid_pct / 100 : frozen_cost);
}
// what a frozen role that skips its dead tiles weighs in the split, in tiles: `live` of its ntasks tiles ran in an earlier step of the same kind
static inline int dead_skip_tasks(int ntasks, int live, const SplitTune& t)
{
    const int lv = std::max(0, std::min(ntasks, live));
    return lv + (int)((long)(ntasks - lv) * t.dead_tile_pct / 100);
}
// workgroups of role r in a split (wg_end: the running ends of the roles' workgroup ranges)
static inline int role_wgs(const int* wg_end, int r) { return wg_end[r] - (r ? wg_end[r - 1] : 0); }

// split num_cu workgroups over roles in proportion to their cost per task (every role gets at least one)
// tasks (optional): per role, the tiles it is expected to RUN (a frozen role under an optimiser mask skips its dead tiles: backward_core), in
// place of ntasks; the cap on a role's workgroups stays with ntasks, the tiles it walks
static inline void split_wgs(int num_cu, int ntasks, int n, const int* cost, int* wg_end, int waves = 8, const int* tasks = nullptr)
{
    int cap = std::max(1, (ntasks + waves - 1) / waves), used = 0;
    double tot = 0;
    auto load = [&](int r) { return (double)cost[r] * (tasks ? std::max(1, tasks[r]) : ntasks); };
    for (int r = 0; r < n; ++r) tot += load(r);
    for (int r = 0; r < n; ++r) {
        int k = std::max(1, (int)((double)num_cu * load(r) / tot));
        k = std::min(k, cap);
        used += k;
        wg_end[r] = used;
    }
}

// Cost-proportional shares, then single workgroups moved from the role that would suffer least to the role that finishes last while
// the modelled makespan (whole tiles per wave x cost) falls: a role's time is a step function of its workgroups, and the
// proportional split alone left the forward 3-5 % behind the best split whenever a role sat just past a step (K3, K4 shard).
static inline void split_wgs_balanced(int num_cu, int ntasks, int n, const int* cost, int* wg_end, int waves = 8, const int* tasks = nullptr)
{
    split_wgs(num_cu, ntasks, n, cost, wg_end, waves, tasks);
    int w[4];
    for (int r = 0; r < n; ++r) w[r] = role_wgs(wg_end, r);
    int used = wg_end[n - 1];
    const int cap = std::max(1, (ntasks + waves - 1) / waves);
    auto t_of = [&](int r, int wr) { return (long)(((tasks ? tasks[r] : ntasks) + waves * wr - 1) / (waves * wr)) * cost[r]; };
    auto last = [&]() { int worst = 0; for (int q = 1; q < n; ++q) if (t_of(q, w[q]) > t_of(worst, w[worst])) worst = q; return worst; };
    for (int r = 0; used < num_cu && r < 8 * n; ++r) {      // hand out what the rounding left, to whoever finishes last
        const int worst = last();
        if (w[worst] >= cap) break;
        ++w[worst]; ++used;
    }
    for (int it = 0; it < 64; ++it) {
        const int worst = last();
        const long cur = t_of(worst, w[worst]);
        if (w[worst] >= cap) break;
        int donor = -1; long best = cur;
        for (int q = 0; q < n; ++q) {
            if (q == worst || w[q] <= 1) continue;
            long m = std::max(t_of(q, w[q] - 1), t_of(worst, w[worst] + 1));
            for (int o = 0; o < n; ++o) if (o != q && o != worst) m = std::max(m, t_of(o, w[o]));
            if (m < best) { best = m; donor = q; }
        }
        if (donor < 0) break;
        --w[donor]; ++w[worst];
    }
    int acc = 0;
    for (int r = 0; r < n; ++r) { acc += w[r]; wg_end[r] = acc; }
}

// Backward with one trainable role: that role advances in whole iterations (8 tasks per workgroup, all its workgroups in
// lockstep), so its time is ceil(groups / workgroups) iterations -- a step function -- while a frozen role's time falls
// smoothly with its workgroups.  Pick the trainable role's share by minimising the modelled makespan instead of in
// proportion to cost (1024 rays: 3 iterations with the proportional 191 workgroups, 2 with 192).
static inline void split_wgs_train(int num_cu, int ntasks, int n, const int* cost, int train_role, int* wg_end, const int* tasks = nullptr)
{
    const int groups = std::max(1, (ntasks + 7) / 8);
    // a frozen role's share of the workgroups the trainable role leaves: in proportion to cost x the tiles it runs
    long fload[3] = {0, 0, 0}, fsum = 0;
    for (int r = 0; r < n; ++r) if (r != train_role) { fload[r] = (long)cost[r] * std::max(1, tasks ? tasks[r] : ntasks); fsum += fload[r]; }
    // For every iteration count the role could run, give it the FEWEST workgroups that reach it: more would not shorten it (its time is
    // a step function) and would starve the frozen roles (1250 rays: 3 iterations need 157 workgroups; the 190 a cost-proportional
    // split hands it left the frozen roles as the kernel's tail, 120 us against 94 us).
    long best = -1; int best_wt = 1;
    const int wt_max = std::min(groups, num_cu - (n - 1));
    for (int iters = (groups + wt_max - 1) / wt_max; iters <= groups; ++iters) {
        const int wt = (groups + iters - 1) / iters;
        if (wt > wt_max) continue;
        long t = (long)iters * cost[train_role];
        const int rest = num_cu - wt;
        for (int r = 0; r < n; ++r) {
            if (r == train_role) continue;
            const int wr = std::max(1, (int)((long)rest * fload[r] / std::max(1L, fsum)));
            t = std::max(t, (long)(((tasks ? tasks[r] : ntasks) + 8 * wr - 1) / (8 * wr)) * cost[r]);
        }
        if (best < 0 || t < best) { best = t; best_wt = wt; }
        if ((long)iters * cost[train_role] > best) break;          // more iterations only get slower from here
    }
    const int rest = num_cu - best_wt;
    int used = 0;
    for (int r = 0; r < n; ++r) {
        int k = r == train_role ? best_wt : std::max(1, (int)((long)rest * fload[r] / std::max(1L, fsum)));
        k = std::min(k, std::max(1, (ntasks + 7) / 8));
        used += k;
        wg_end[r] = used;
    }
}

// predicted time of a split in the cost units of its roles: every wave of a role walks ceil(tiles / waves) tiles
static inline long split_makespan(int ntasks, int n, const int* cost, const int* wg_end, int waves = 8, const int* tasks = nullptr)
{
    long t = 0;
    for (int r = 0; r < n; ++r) {
        const int w = std::max(1, role_wgs(wg_end, r));
        t = std::max(t, (long)(((tasks ? tasks[r] : ntasks) + waves * w - 1) / (waves * w)) * cost[r]);
    }
    return t;
}

// Forward of a stage with the middle and the fine decoder (and the colour one: `colour`): middle + fine as ONE role, or a role per decoder.
// A merged tile is two decoders long, so small batches quantise worse (K2: 3 000 tiles on 256 workgroups -- forward 37.7 us as three roles,
// 40.2 as two): take the form whose split predicts the shorter launch.  no_occ_role 1: never merged (also: the launch cannot be), 2: always
struct FwdPlan { bool merged; int n, wg_end[3]; };      // merged without colour: n = 1, wg_end[1] = wg_end[0] (the kernel's colour role is empty)
static inline FwdPlan plan_fwd(int num_cu, int ntasks, bool colour, const SplitTune& t, int no_occ_role)
{
    FwdPlan P3 = {false, colour ? 3 : 2, {0, 0, 0}};
    int cost3[3];
    for (int r = 0; r < P3.n; ++r) cost3[r] = fwd_role_cost(1 + r, t);
    if (no_occ_role != 2) split_wgs_balanced(num_cu, ntasks, P3.n, cost3, P3.wg_end, 8);
    if (no_occ_role == 1) return P3;
    FwdPlan P = {true, colour ? 2 : 1, {0, 0, 0}};
    const int cost[2] = {fwd_occ_role_cost(t), fwd_role_cost(3, t)};
    split_wgs_balanced(num_cu, ntasks, P.n, cost, P.wg_end, 8);
    if (!colour) P.wg_end[1] = P.wg_end[0];
    if (no_occ_role != 2 && split_makespan(ntasks, P.n, cost, P.wg_end) > split_makespan(ntasks, P3.n, cost3, P3.wg_end)) return P3;
    return P;
}

// Backward: one trainable role among several -> split_wgs_train; else the balanced split over workgroups of `waves` waves (8, or the frozen
// kernel's when the launch has no trainable role and no ray gradients).  tasks: see split_wgs
static inline void plan_bwd(int num_cu, int ntasks, int n, const int* cost, int train_role, int waves, const int* tasks, int* wg_end)
{
    if (train_role >= 0 && n > 1) split_wgs_train(num_cu, ntasks, n, cost, train_role, wg_end, tasks);
    else split_wgs_balanced(num_cu, ntasks, n, cost, wg_end, waves, tasks);
}
