// nsk_split.h -- how a decoder launch divides its workgroups over its roles, and which launch goes out: cost model, split arithmetic and the
// backward's launch form in host integers, nothing of HIP (host/test/split_test.cpp builds it with a plain host compiler: tests/test_split_cpu.py)
//   split_wgs, split_wgs_balanced, split_wgs_train, split_makespan      the split arithmetic
//   plan_fwd, plan_bwd                                                  which split a forward / backward launch takes (and the forward's form)
//   bwd_form, bwd_deal_role, bwd_grid                                   which backward launch goes out, with which riders, on how many workgroups
//   median_form                                                         which of the Tracker's median forms runs in front of it
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

// ---- The backward's launch form.  One decision, taken once in backward_core (nsk.hip) from the facts below; the launch, the liveness pass, the
// riders and nsk_debug_last_split all read its answer.
//
//   kernel              runs when                                                                      waves  skip  deal  scan rider
//   BWD_NONE            no decoder of the stage has a gradient to compute                              -      -     -     -
//   BWD_SEPARATE        deterministic mode; or several trainable roles, or the fine one (its body is   8      -     -     -
//                       not part of k_decode_bwd_multi): one launch per decoder, in a fixed order
//   BWD_TRACK           the Tracker handed in its deferred median mask (see median_form)               8      -     -     -
//   BWD_MULTI_FULL      bwd_mode 0: every chain on the fp32 MFMA; _RAYS: with ray gradients            8      -     -     -
//   BWD_FROZEN          no trainable role, no ray gradients, no_frozen_kernel off: 16-wave workgroups  16     yes   -     yes
//   BWD_MULTI_RAYS      ray gradients (bundle adjustment; the Tracker without a mask)                  8      -     -     -
//   BWD_MULTI           the rest (one trainable role beside frozen ones: the Mapper's colour stage)    8      yes   yes   yes
//   BWD_MULTI_DEAL      BWD_MULTI with at least one role that claims its tiles from a cursor: bwd_deal_role says which, once the split is
//                       known, and bwd_launch_kernel then names the kernel that goes out
//
// skip (frozen roles under an optimiser mask skip their dead tiles) also needs grid gradients and no_dead_skip off: with ray gradients d/dp
// flows through every sample.  deal also needs static_deal off.  The scan rider is the next batch's cell-sort scan (prep_ride_scan).
static const int BWD_FROZEN_WAVES = 16;             // = NSK_FROZEN_NW (nsk_device.h; nsk.hip asserts it)
static const int BWD_MEDIAN_MAX_RAYS = 1024;        // = NSK_MEDIAN_FUSED_MAX

enum BwdKernel { BWD_NONE = 0, BWD_SEPARATE, BWD_TRACK, BWD_MULTI_FULL, BWD_MULTI_FULL_RAYS, BWD_FROZEN, BWD_MULTI_RAYS, BWD_MULTI, BWD_MULTI_DEAL };

struct BwdFormIn {
    int n = 0, which[3] = {0, 0, 0}, train[3] = {0, 0, 0};      // the collected roles, in launch order
    bool rays = false, grids = false;                            // NSK_GRAD_RAYS, NSK_GRAD_GRIDS
    bool full = false, deterministic = false;                    // bwd_mode == 0; the deterministic debug mode
    bool track = false;                                          // a deferred median mask was handed in
    int N = 0;                                                   // rays
    int no_frozen_kernel = 0, no_dead_skip = 0, static_deal = 0;      // nsk_set_tuning keys of the same names (deal_min_rounds: bwd_deal_role)
};

struct BwdForm {
    BwdKernel kernel = BWD_NONE;
    int train_role = -1;              // the one trainable role; -1: none; -2: several, or the fine decoder (-> BWD_SEPARATE)
    int waves = 8;                    // per workgroup
    bool skip_eligible = false, deal_eligible = false, scan_may_ride = false;
    int scan_halves = 2;              // the scan rider's 256-cell chunks per workgroup
    bool mask_ok = true;              // false: a deferred mask with inputs the Tracker's launch does not serve
};

static inline BwdForm bwd_form(const BwdFormIn& in)
{
    BwdForm F;
    for (int r = 0; r < in.n; ++r) if (in.train[r]) F.train_role = (F.train_role == -1 && in.which[r] != 2) ? r : -2;
    F.mask_ok = !in.track || (F.train_role == -1 && in.rays && !in.deterministic && !in.full && in.n > 0 && in.N <= BWD_MEDIAN_MAX_RAYS);
    if (in.n == 0 || !F.mask_ok) return F;
    if (in.deterministic || F.train_role == -2) { F.kernel = BWD_SEPARATE; return F; }
    if (in.track) F.kernel = BWD_TRACK;
    else if (in.full) F.kernel = in.rays ? BWD_MULTI_FULL_RAYS : BWD_MULTI_FULL;
    else if (in.rays) F.kernel = BWD_MULTI_RAYS;
    else F.kernel = (F.train_role == -1 && !in.no_frozen_kernel) ? BWD_FROZEN : BWD_MULTI;
    const bool plain = F.kernel == BWD_FROZEN || F.kernel == BWD_MULTI;      // two-piece chains, no ray gradients, no mask of the Tracker's
    if (F.kernel == BWD_FROZEN) { F.waves = BWD_FROZEN_WAVES; F.scan_halves = BWD_FROZEN_WAVES / 4; }
    F.skip_eligible = plain && in.grids && !in.no_dead_skip;
    // Dealing only where a wave has rounds enough for a claimed tail to even out (bwd_deal_role), and not in the 16-wave kernel: a role there is
    // ~2000 waves of ~8 tiles, every wave claims at least twice, and adds on one address serialise at ~25 ns (K3 fine stage 83 -> 114 us with
    // per-wave claims)
    F.deal_eligible = F.skip_eligible && F.kernel == BWD_MULTI && !in.static_deal;
    F.scan_may_ride = plain;
    return F;
}

// the form as nsk_debug_last_split reports it (NSK_SPLIT_BWD_*, include/nsk.h; 0: no launch)
static inline int bwd_split_form(BwdKernel k)
{
    switch (k) {
    case BWD_NONE: return 0;
    case BWD_SEPARATE: return 1;
    case BWD_MULTI_RAYS: case BWD_MULTI: case BWD_MULTI_DEAL: return 2;
    case BWD_MULTI_FULL: case BWD_MULTI_FULL_RAYS: return 3;
    case BWD_FROZEN: return 4;
    case BWD_TRACK: return 5;
    }
    return 0;
}

// Does role r claim its tiles from its cursor (k_decode_bwd_multi_deal)?  counted: the role skips dead tiles (bwd_liveness).  K2 and the K4 shard
// (11 and 10 rounds per wave, the trainable role's iterations being the launch) gain nothing, and the K4 shard pays 1.2 - 1.6 us for the claims.
// deal_min_rounds: the nsk_set_tuning key.
static inline bool bwd_deal_role(int ntasks, int role_workgroups, bool counted, const BwdForm& F, int deal_min_rounds)
{
    if (!F.deal_eligible || !counted) return false;
    return (ntasks + role_workgroups * 8 - 1) / (role_workgroups * 8) >= deal_min_rounds;
}
// the kernel that goes out: the form's, or the dealing one when a role claims (any_dealt: bwd_deal_role of some role; only BWD_MULTI is eligible)
static inline BwdKernel bwd_launch_kernel(const BwdForm& F, bool any_dealt) { return any_dealt ? BWD_MULTI_DEAL : F.kernel; }

// workgroups of the launch: the roles', then the riders (the Tracker's one rider finds the median and sums the loss, asked for or not)
static inline int bwd_grid(const BwdForm& F, const int* wg_end, int n, int scan_wgs, int loss_wg)
{
    return wg_end[n - 1] + (F.kernel == BWD_TRACK ? 1 : scan_wgs + loss_wg);
}
// one launch per decoder (BWD_SEPARATE): persistent, one workgroup per CU; in the deterministic mode one workgroup, its waves one after the other
static inline int bwd_separate_grid(int num_cu, int ntasks, bool deterministic)
{
    return deterministic ? 1 : std::max(1, std::min((ntasks + 7) / 8, num_cu));
}

// ---- The Tracker's median threshold (handle_dynamic: rays whose depth residual exceeds 10 x the batch median leave the loss), in front of the
// backward.  Which form runs when:
//   MEDIAN_NONE      handle_dynamic off: composite mode 3, no threshold
//   MEDIAN_DEFERRED  ray gradients, frozen decoders, two-piece chains, at most BWD_MEDIAN_MAX_RAYS rays (the Tracker as the reference runs it):
//                    composite mode 5 writes residuals and seeds, the backward's workgroups find the median and apply the mask (BWD_TRACK)
//   MEDIAN_BARRIER   else, while the compositing grid is at most one workgroup per CU, i.e. certainly resident as a whole: composite mode 4
//                    (residuals -> grid barrier -> median -> loss and backward) in one launch
//   MEDIAN_THREE     else, in the deterministic mode and under no_fused_median: a forward, the median's own launch, composite mode 3
// no_deferred_median leaves out the deferred form alone.  any_trainable: a decoder of the stage is trainable and the flags ask for decoder
// gradients -- the rule by which collect_bwd_roles (nsk.hip) marks a role trainable; the two must agree, or bwd_form refuses the mask.
// (Round 3 tried ONE 16-wave workgroup for up to 256 rays -- render, select the median in LDS, render again, no grid barrier: 70 us at 200 rays
// against 21, a wave's rays run one after the other at ~2.5 us each.)
enum MedianForm { MEDIAN_NONE = 0, MEDIAN_THREE, MEDIAN_BARRIER, MEDIAN_DEFERRED };
static inline MedianForm median_form(bool handle_dynamic, bool deterministic, int no_fused_median, int no_deferred_median, int N, int num_cu,
                                     bool rays, bool full, bool any_trainable)
{
    if (!handle_dynamic) return MEDIAN_NONE;
    if (deterministic || no_fused_median || N > BWD_MEDIAN_MAX_RAYS) return MEDIAN_THREE;
    if (!no_deferred_median && rays && !full && !any_trainable) return MEDIAN_DEFERRED;
    return (N + 3) / 4 <= num_cu ? MEDIAN_BARRIER : MEDIAN_THREE;
}
