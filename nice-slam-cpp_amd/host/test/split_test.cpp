// The workgroup-split planner of the decoder launches (csrc/nsk_split.h) on the CPU: no torch, no HIP.  tests/test_split_cpu.py runs it.
//   split_test <table>   the literal cases below, then every row of the recorded table (tests/golden/wg_splits.txt) recomputed and compared,
//                        then the planner swept at the extremes of its tuning keys (knob_sweep: properties, nothing recorded), then the
//                        backward's launch form and the Tracker's median form over every combination of their inputs (form_sweep: properties)
//   split_test --dump    prints the sweep in the table's format (how the table was recorded: see the table's header)
// Row: <fn> <num_cu> <ntasks> <n> <waves> <train_role>  c0 c1 c2  t0 t1 t2 | w0 w1 w2 <makespan>      fn: S split_wgs, B split_wgs_balanced,
// T split_wgs_train; t0 = -1: no tasks; unused columns 0; w: workgroups per role; makespan: split_makespan of that split (same waves and tasks)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nsk_split.h"

static const int NUM_CU = 256;
static int failures = 0;

struct Row { char fn; int num_cu, ntasks, n, waves, train_role, cost[3], tasks[3], w[3]; long makespan; };

static void compute(Row& R)
{
    int wg_end[3] = {0, 0, 0};
    const int* tasks = R.tasks[0] < 0 ? nullptr : R.tasks;
    if (R.fn == 'S') split_wgs(R.num_cu, R.ntasks, R.n, R.cost, wg_end, R.waves, tasks);
    else if (R.fn == 'B') split_wgs_balanced(R.num_cu, R.ntasks, R.n, R.cost, wg_end, R.waves, tasks);
    else split_wgs_train(R.num_cu, R.ntasks, R.n, R.cost, R.train_role, wg_end, tasks);
    for (int r = 0; r < 3; ++r) R.w[r] = r < R.n ? role_wgs(wg_end, r) : 0;
    R.makespan = split_makespan(R.ntasks, R.n, R.cost, wg_end, R.waves, tasks);
}

static void print_row(FILE* f, const Row& R)
{
    fprintf(f, "%c %d %d %d %d %d  %d %d %d  %d %d %d | %d %d %d %ld\n", R.fn, R.num_cu, R.ntasks, R.n, R.waves, R.train_role, R.cost[0], R.cost[1],
            R.cost[2], R.tasks[0], R.tasks[1], R.tasks[2], R.w[0], R.w[1], R.w[2], R.makespan);
}

// every role has a workgroup and none more than the tiles it walks fill (wg_end increasing follows from the first)
static bool within_caps(const Row& R)
{
    const int cap = std::max(1, (R.ntasks + R.waves - 1) / R.waves);
    for (int r = 0; r < R.n; ++r) if (R.w[r] < 1 || R.w[r] > cap) return false;
    return true;
}

static std::vector<int> sweep_tiles()
{
    std::vector<int> v;
    for (int t = 1; t <= 64; ++t) v.push_back(t);
    for (int p = 7; p <= 20; ++p) for (int d = -1; d <= 1; ++d) v.push_back((1 << p) + d);
    return v;
}

static Row make_row(char fn, int ntasks, int n, int waves, int train_role, const int* cost, bool with_tasks)
{
    Row R;
    memset(&R, 0, sizeof(R));
    R.fn = fn; R.num_cu = NUM_CU; R.ntasks = ntasks; R.n = n; R.waves = waves; R.train_role = train_role;
    const int part[3] = {ntasks, ntasks * 3 / 10, ntasks / 8};        // a role that runs everything, one that skips most, one that skips nearly all
    for (int r = 0, f = 1; r < n; ++r) {
        R.cost[r] = fn == 'T' ? (r == train_role ? 1000 : cost[r]) : cost[r];
        R.tasks[r] = fn == 'T' ? (r == train_role ? ntasks : part[f++]) : part[r];
    }
    if (!with_tasks) { R.tasks[0] = -1; R.tasks[1] = R.tasks[2] = 0; }
    return R;
}

static int dump()
{
    static const int fwd[3] = {240, 292, 248}, frozen[3] = {205, 205, 205};
    long rows = 0, bad = 0;
    for (int ntasks : sweep_tiles())
        for (int n = 1; n <= 3; ++n)
            for (int tk = 0; tk < 2; ++tk) {
                std::vector<Row> v;
                for (int waves = 8; waves <= 16; waves += 8) {
                    v.push_back(make_row('S', ntasks, n, waves, -1, waves == 8 ? fwd : frozen, tk));
                    v.push_back(make_row('B', ntasks, n, waves, -1, fwd, tk));
                    v.push_back(make_row('B', ntasks, n, waves, -1, frozen, tk));
                }
                for (int tr = 0; tr < n; ++tr) v.push_back(make_row('T', ntasks, n, 8, tr, frozen, tk));
                for (Row& R : v) { compute(R); print_row(stdout, R); ++rows; if (!within_caps(R)) { ++bad; fprintf(stderr, "caps: "); print_row(stderr, R); } }
            }
    fprintf(stderr, "%ld rows, %ld outside [1, cap]\n", rows, bad);
    return 0;
}

static void expect(const char* what, char fn, int ntasks, int n, int waves, int train_role, const int* cost, const int* tasks, const int* want, long want_makespan = -1)
{
    Row R;
    memset(&R, 0, sizeof(R));
    R.fn = fn; R.num_cu = NUM_CU; R.ntasks = ntasks; R.n = n; R.waves = waves; R.train_role = train_role; R.tasks[0] = -1;
    for (int r = 0; r < n; ++r) { R.cost[r] = cost[r]; if (tasks) R.tasks[r] = tasks[r]; }
    compute(R);
    bool ok = want_makespan < 0 || R.makespan == want_makespan;
    for (int r = 0; r < n; ++r) ok = ok && R.w[r] == want[r];
    if (!ok) { ++failures; fprintf(stderr, "FAIL %s: got ", what); print_row(stderr, R); }
}

static void literal_cases()
{
    // the backward of the colour stage: roles {colour trainable, fine, middle}, 48 samples per ray -> 3 tiles per ray
    const int ctrain[3] = {1000, 205, 205};
    const int t64[3] = {24, 24, 24}, t1000[3] = {188, 34, 34}, t1024[3] = {192, 32, 32}, t1250[3] = {157, 49, 49}, t5000[3] = {171, 42, 42};
    expect("train 64 rays", 'T', 192, 3, 8, 0, ctrain, nullptr, t64);
    expect("train 1000 rays", 'T', 3000, 3, 8, 0, ctrain, nullptr, t1000);
    expect("train 1024 rays (2 iterations need 192 workgroups)", 'T', 3072, 3, 8, 0, ctrain, nullptr, t1024);
    expect("train 1250 rays (3 iterations need 157 workgroups)", 'T', 3750, 3, 8, 0, ctrain, nullptr, t1250);
    expect("train 5000 rays", 'T', 15000, 3, 8, 0, ctrain, nullptr, t5000);
    const int live[3] = {3072, 900, 400}, tlive[3] = {192, 44, 19};
    expect("train 1024 rays, live counts", 'T', 3072, 3, 8, 0, ctrain, live, tlive);
    // two frozen roles on the 16-wave kernel
    const int fr[2] = {205, 205}, f192[2] = {12, 12}, f128[2] = {128, 128};
    expect("frozen 192 tiles", 'B', 192, 2, 16, -1, fr, nullptr, f192);
    expect("frozen 3072 tiles", 'B', 3072, 2, 16, -1, fr, nullptr, f128);
    expect("frozen 15000 tiles", 'B', 15000, 2, 16, -1, fr, nullptr, f128);
    // the forward's three roles
    const int fw[3] = {240, 292, 248}, one[3] = {1, 1, 1}, w3000[3] = {78, 95, 83}, w15000[3] = {79, 95, 82};
    expect("forward 1 tile", 'B', 1, 3, 8, -1, fw, nullptr, one, 292);
    expect("forward 7 tiles", 'B', 7, 3, 8, -1, fw, nullptr, one, 292);
    expect("forward 3000 tiles", 'B', 3000, 3, 8, -1, fw, nullptr, w3000, 1240);
    expect("forward 15000 tiles", 'B', 15000, 3, 8, -1, fw, nullptr, w15000, 5840);
    const int mg[2] = {460, 248}, wm[2] = {167, 89};
    expect("forward merged 3000 tiles", 'B', 3000, 2, 8, -1, mg, nullptr, wm, 1380);
    expect("one role, one tile", 'B', 1, 1, 8, -1, fw, nullptr, one);

    // the forward's choice: 3 000 tiles predict 1 380 merged against 1 240 as three roles (K2) -> three roles, with their split
    const SplitTune T;
    FwdPlan P = plan_fwd(NUM_CU, 3000, true, T, 0);
    if (P.merged || P.n != 3 || P.wg_end[0] != 78 || P.wg_end[1] != 78 + 95 || P.wg_end[2] != 78 + 95 + 83) { ++failures; fprintf(stderr, "FAIL plan_fwd 3000 tiles\n"); }
    P = plan_fwd(NUM_CU, 3000, true, T, 2);
    if (!P.merged || P.n != 2 || P.wg_end[0] != 167 || P.wg_end[1] != 167 + 89) { ++failures; fprintf(stderr, "FAIL plan_fwd 3000 tiles, always merged\n"); }
    P = plan_fwd(NUM_CU, 3000, false, T, 2);
    if (!P.merged || P.n != 1 || P.wg_end[1] != P.wg_end[0]) { ++failures; fprintf(stderr, "FAIL plan_fwd without colour\n"); }
    // the cost model's built-in values and the keys that override them
    SplitTune U;
    bool ok = fwd_role_cost(0, U) == 96 && fwd_role_cost(1, U) == 240 && fwd_role_cost(2, U) == 292 && fwd_role_cost(3, U) == 248 && fwd_occ_role_cost(U) == 460;
    ok = ok && bwd_role_cost(true, 3, false, U) == 1000 && bwd_role_cost(false, 2, false, U) == 205 && bwd_role_cost(false, 1, true, U) == 330;
    ok = ok && dead_skip_tasks(3072, 900, U) == 900 + (3072 - 900) * 12 / 100 && dead_skip_tasks(100, 500, U) == 100 && dead_skip_tasks(100, -3, U) == 12;
    U.fwd_fine_cost = 300; U.fwd_color_cost = 250; U.fwd_occ_cost = 470; U.frozen_cost = 220; U.frozen_cost_rays = 340; U.frozen_mid_pct = 150; U.dead_tile_pct = 0;
    ok = ok && fwd_role_cost(1, U) == 240 && fwd_role_cost(2, U) == 300 && fwd_role_cost(3, U) == 250 && fwd_occ_role_cost(U) == 470;
    ok = ok && bwd_role_cost(false, 2, false, U) == 220 && bwd_role_cost(false, 1, false, U) == 330 && bwd_role_cost(false, 3, true, U) == 340 && dead_skip_tasks(100, 40, U) == 40;
    if (!ok) { ++failures; fprintf(stderr, "FAIL cost model\n"); }
    // the backward's choice: one trainable role among several -> the iteration-count split; alone, or none -> the balanced one on the given waves
    int a[3], b[3];
    plan_bwd(NUM_CU, 3072, 3, ctrain, 0, 8, nullptr, a); split_wgs_train(NUM_CU, 3072, 3, ctrain, 0, b);
    ok = !memcmp(a, b, sizeof(a));
    plan_bwd(NUM_CU, 3072, 2, fr, -1, 16, nullptr, a); split_wgs_balanced(NUM_CU, 3072, 2, fr, b, 16);
    ok = ok && !memcmp(a, b, 2 * sizeof(int));
    plan_bwd(NUM_CU, 3072, 1, ctrain, 0, 8, nullptr, a); split_wgs_balanced(NUM_CU, 3072, 1, ctrain, b, 8);
    ok = ok && a[0] == b[0];
    if (!ok) { ++failures; fprintf(stderr, "FAIL plan_bwd\n"); }
}

// The planner at the extremes of its nsk_set_tuning keys, through the entry points the launches use (plan_fwd, plan_bwd with bwd_role_cost and
// dead_skip_tasks): properties only, nothing recorded.  Every role in [1, cap], wg_end strictly increasing, and the trainable role within the
// num_cu - (n - 1) rows its per-workgroup gradient slabs have.
static long knob_sweep()
{
    long plans = 0;
    auto bad = [&](const char* what, int num_cu, int ntasks, int n, const int* wg_end) {
        if (++failures < 20) fprintf(stderr, "FAIL knob sweep %s: num_cu %d tiles %d n %d -> ends %d %d %d\n", what, num_cu, ntasks, n, wg_end[0], n > 1 ? wg_end[1] : 0, n > 2 ? wg_end[2] : 0);
    };
    auto check = [&](const char* what, int num_cu, int ntasks, int n, int waves, int train_role, const int* wg_end) {
        ++plans;
        const int cap = std::max(1, (ntasks + waves - 1) / waves);
        for (int r = 0; r < n; ++r) {
            const int w = role_wgs(wg_end, r);
            if (w < 1 || w > cap || (r == train_role && w > num_cu - (n - 1))) { bad(what, num_cu, ntasks, n, wg_end); return; }      // (w >= 1 for every r: strictly increasing)
        }
    };
    std::vector<int> tiles;
    for (int t = 1; t <= 200; ++t) tiles.push_back(t);
    for (int t = 203; t <= 3000; t += 7) tiles.push_back(t);
    tiles.push_back(999); tiles.push_back(3000);
    static const int costs[3] = {0, 1, 100000}, pcts[3] = {10, 100, 1000}, dead[3] = {-1, 0, 100};      // dead -1: no live counts (tasks = nullptr)
    static const int cus[2] = {256, 104};
    for (int num_cu : cus)
        for (int ntasks : tiles) {
            // backward: roles in launch order (colour, fine, middle), or (fine, middle)
            for (int n = 2; n <= 3; ++n)
                for (int form = 0; form < 5; ++form) {        // 0 frozen kernel (16 waves), 1 frozen roles in the multi kernel, 2 frozen with ray gradients, 3 trainable, 4 trainable with ray gradients
                    const bool rays = form == 2 || form == 4;
                    const int train_role = form >= 3 ? 0 : -1, waves = form == 0 ? 16 : 8;
                    for (int fc : costs) for (int pct : pcts) for (int dp : dead) {
                        SplitTune T;
                        T.frozen_cost = fc; T.frozen_cost_rays = fc; T.frozen_mid_pct = pct; if (dp >= 0) T.dead_tile_pct = dp;
                        int cost[3], tasks[3], wg_end[3] = {0, 0, 0};
                        for (int r = 0; r < n; ++r) {
                            const int w = n == 3 ? 3 - r : 2 - r;
                            cost[r] = bwd_role_cost(r == train_role, w, rays, T);
                            tasks[r] = r == train_role ? ntasks : dead_skip_tasks(ntasks, r == n - 1 ? ntasks / 8 : ntasks * 3 / 10, T);
                        }
                        plan_bwd(num_cu, ntasks, n, cost, train_role, waves, dp >= 0 && !rays ? tasks : nullptr, wg_end);
                        check("plan_bwd", num_cu, ntasks, n, waves, train_role, wg_end);
                    }
                }
            // forward: the three keys at default / 1 / 100000, with and without the colour role, every no_occ_role
            for (int fo : costs) for (int ff : costs) for (int fcl : costs)
                for (int colour = 0; colour < 2; ++colour)
                    for (int nor = 0; nor <= 2; ++nor) {
                        SplitTune T;
                        T.fwd_occ_cost = fo; T.fwd_fine_cost = ff; T.fwd_color_cost = fcl;
                        const FwdPlan P = plan_fwd(num_cu, ntasks, colour != 0, T, nor);
                        const int want_n = P.merged ? (colour ? 2 : 1) : (colour ? 3 : 2);
                        if (P.n != want_n || (nor == 1 && P.merged) || (nor == 2 && !P.merged)) bad("plan_fwd form", num_cu, ntasks, P.n, P.wg_end);
                        check("plan_fwd", num_cu, ntasks, P.n, 8, -1, P.wg_end);
                    }
        }
    // the costs at the top of the range nsk_set_tuning accepts: the middle role's cost stays an int (1 000 000 x 1000 / 100 < 2^31)
    SplitTune T;
    T.frozen_cost = T.frozen_cost_rays = 1000000; T.frozen_mid_pct = 1000;
    if (bwd_role_cost(false, 1, false, T) != 10000000 || bwd_role_cost(false, 1, true, T) != 10000000) { ++failures; fprintf(stderr, "FAIL knob sweep: cost at the top of the range\n"); }
    return plans;
}

// The backward's launch form (bwd_form, bwd_deal_role, bwd_grid) and the Tracker's median form (median_form) over every combination of their
// boolean inputs, the role sets of the four stages x their trainable subsets, N in {1, 200, 1024, 1025} and num_cu in {50, 256}.  The properties
// are those the launch code stated in its comments before the decision had one home: they are written from the inputs, not from the functions.
static long form_sweep()
{
    long forms = 0;
    static const int stage_dec[4][3] = {{0, -1, -1}, {1, -1, -1}, {1, 2, -1}, {1, 2, 3}};      // the decoders a stage runs
    static const int Ns[4] = {1, 200, 1024, 1025}, cus[2] = {50, 256};
    auto bad = [&](const char* what, const BwdFormIn& in, const BwdForm& F) {
        if (++failures < 20)
            fprintf(stderr, "FAIL form sweep %s: n %d which %d %d %d train %d %d %d rays %d grids %d full %d det %d track %d N %d knobs %d %d %d -> kernel %d\n", what, in.n,
                    in.which[0], in.which[1], in.which[2], in.train[0], in.train[1], in.train[2], in.rays, in.grids, in.full, in.deterministic, in.track, in.N,
                    in.no_frozen_kernel, in.no_dead_skip, in.static_deal, (int)F.kernel);
    };
    for (int stage = 0; stage < 4; ++stage)
    for (int tmask = 0; tmask < 8; ++tmask)          // bit q: decoder stage_dec[stage][q] is trainable and the flags ask for decoder gradients
    for (int bits = 0; bits < 256; ++bits)
    for (int N : Ns) {
        if (tmask >> (stage < 2 ? 1 : stage)) continue;      // (bits of decoders the stage does not have)
        BwdFormIn in;
        in.rays = bits & 1; in.grids = bits & 2; in.full = bits & 4; in.deterministic = bits & 8; in.track = bits & 16;
        in.no_frozen_kernel = (bits >> 5) & 1; in.no_dead_skip = (bits >> 6) & 1; in.static_deal = (bits >> 7) & 1; in.N = N;
        int ntrain = 0; bool fine_train = false;
        for (int q = 2; q >= 0; --q) {                  // launch order: colour, fine, middle (collect_bwd_roles)
            const int w = stage_dec[stage][q];
            if (w < 0) continue;
            const bool train = (tmask >> q) & 1;
            if (!train && !in.grids && !in.rays) continue;
            in.which[in.n] = w; in.train[in.n] = train; ++in.n;
            ntrain += train; fine_train = fine_train || (train && w == 2);
        }
        const BwdForm F = bwd_form(in);
        ++forms;
        // a deferred mask is legal only for the Tracker's launch; an illegal one launches nothing
        const bool mask_ok = !in.track || (ntrain == 0 && in.rays && !in.deterministic && !in.full && in.n > 0 && N <= 1024);
        if (F.mask_ok != mask_ok) bad("mask_ok", in, F);
        if (!mask_ok) { if (F.kernel != BWD_NONE || F.skip_eligible || F.deal_eligible || F.scan_may_ride) bad("illegal mask launches", in, F); continue; }
        // exactly one kernel
        const bool separate = in.n > 0 && (in.deterministic || ntrain > 1 || fine_train);
        if ((F.kernel == BWD_NONE) != (in.n == 0)) bad("none", in, F);
        if ((F.kernel == BWD_SEPARATE) != separate) bad("separate", in, F);
        if (F.kernel == BWD_TRACK && !(in.track && in.rays && ntrain == 0 && !in.deterministic && !in.full && N <= 1024)) bad("track", in, F);
        if (in.track && F.kernel != BWD_TRACK) bad("a legal mask takes the Tracker's launch", in, F);
        const bool frozen = in.n > 0 && ntrain == 0 && !in.rays && !in.full && !in.no_frozen_kernel && !separate;
        if ((F.kernel == BWD_FROZEN) != frozen) bad("frozen", in, F);
        if ((F.kernel == BWD_MULTI_FULL) != (in.n > 0 && !separate && in.full && !in.rays)) bad("full", in, F);
        if ((F.kernel == BWD_MULTI_FULL_RAYS) != (in.n > 0 && !separate && in.full && in.rays)) bad("full<rays>", in, F);
        if ((F.kernel == BWD_MULTI_RAYS) != (in.n > 0 && !separate && !in.full && !in.track && in.rays)) bad("multi<rays>", in, F);
        if ((F.kernel == BWD_MULTI) != (in.n > 0 && !separate && !in.full && !in.rays && !frozen)) bad("multi", in, F);
        if (F.kernel == BWD_MULTI_DEAL) bad("dealing is decided after the split", in, F);
        // the one trainable role, where the launch has roles
        if (F.kernel != BWD_NONE && F.kernel != BWD_SEPARATE) {
            int want = -1;
            for (int r = 0; r < in.n; ++r) if (in.train[r]) want = r;
            if (F.train_role != want) bad("train_role", in, F);
        }
        // workgroup shape, riders
        if (F.waves != (frozen ? 16 : 8) || F.scan_halves != (frozen ? 4 : 2)) bad("waves", in, F);
        if (F.skip_eligible && !(in.grids && !in.rays && !in.full && !in.track && !in.no_dead_skip && !separate)) bad("skip_eligible", in, F);
        if (F.skip_eligible != (in.n > 0 && in.grids && !in.rays && !in.full && !in.track && !in.no_dead_skip && !separate)) bad("skip_eligible (iff)", in, F);
        if (F.deal_eligible && !(F.skip_eligible && F.kernel != BWD_FROZEN && !in.static_deal)) bad("deal_eligible", in, F);
        if (F.deal_eligible != (F.skip_eligible && !frozen && !in.static_deal)) bad("deal_eligible (iff)", in, F);
        if (F.scan_may_ride && (in.rays || in.full || in.track || separate)) bad("scan_may_ride", in, F);
        if (F.scan_may_ride != (in.n > 0 && !in.rays && !in.full && !separate)) bad("scan_may_ride (iff)", in, F);
        // what nsk_debug_last_split reports (NSK_SPLIT_BWD_*: include/nsk.h)
        const int split_form = in.n == 0 ? 0 : (separate ? 1 : (in.track ? 5 : (in.full ? 3 : (frozen ? 4 : 2))));
        if (bwd_split_form(F.kernel) != split_form) bad("split form", in, F);
        // dealing: a counted role of an eligible launch with at least deal_min_rounds rounds of 8 waves (here 12: 96 tiles per workgroup)
        for (int wgs = 1; wgs <= 3; ++wgs)
            for (int ntasks : {96 * wgs - 8, 96 * wgs - 7, 96 * wgs})           // 11 rounds, 12 rounds (the first tile of the twelfth), 12 rounds
                for (int counted = 0; counted < 2; ++counted) {
                    const int rounds = (ntasks + 8 * wgs - 1) / (8 * wgs);
                    const bool deals = bwd_deal_role(ntasks, wgs, counted != 0, F, 12);
                    if (deals != (F.deal_eligible && counted && rounds >= 12)) bad("bwd_deal_role", in, F);
                    if (bwd_launch_kernel(F, deals) != (deals ? BWD_MULTI_DEAL : F.kernel) || (deals && F.kernel != BWD_MULTI)) bad("bwd_launch_kernel", in, F);
                }
        // the grid: the roles' workgroups, then the Tracker's one rider or the scan's and the loss's
        if (in.n > 0 && !separate) {
            const int wg_end[3] = {5, 9, 12};
            for (int scan = 0; scan <= 3; scan += 3)
                for (int loss = 0; loss < 2; ++loss)
                    if (bwd_grid(F, wg_end, in.n, scan, loss) != wg_end[in.n - 1] + (in.track ? 1 : scan + loss)) bad("bwd_grid", in, F);
        }
        // the median in front of the launch (track unset above: the form decides whether a mask is handed in)
        if (in.track || in.n == 0) continue;
        for (int num_cu : cus)
            for (int mb = 0; mb < 8; ++mb) {
                const bool hd = mb & 1; const int no_fused = (mb >> 1) & 1, no_deferred = (mb >> 2) & 1;
                const MedianForm m = median_form(hd, in.deterministic, no_fused, no_deferred, N, num_cu, in.rays, in.full, ntrain > 0);
                ++forms;
                if ((m == MEDIAN_NONE) != !hd) bad("median none", in, F);
                if (hd && no_fused && m != MEDIAN_THREE) bad("no_fused_median", in, F);
                if (hd && in.deterministic && m != MEDIAN_THREE) bad("median, deterministic", in, F);
                if (m == MEDIAN_DEFERRED) {
                    BwdFormIn tin = in;
                    tin.track = true;
                    if (no_deferred || !bwd_form(tin).mask_ok || bwd_form(tin).kernel != BWD_TRACK) bad("deferred without the Tracker's launch", in, F);
                }
                if (m == MEDIAN_BARRIER && !((N + 3) / 4 <= num_cu && N <= 1024)) bad("barrier beyond one workgroup per CU", in, F);
                // the fastest legal form runs: deferred where the backward takes the mask, else the barrier where the grid is resident
                const bool fused_ok = hd && !in.deterministic && !no_fused && N <= 1024;
                const bool can_defer = fused_ok && !no_deferred && in.rays && !in.full && ntrain == 0;
                const MedianForm want = !hd ? MEDIAN_NONE : (can_defer ? MEDIAN_DEFERRED : (fused_ok && (N + 3) / 4 <= num_cu ? MEDIAN_BARRIER : MEDIAN_THREE));
                if (m != want) bad("median form", in, F);
            }
    }
    // the forms of the steps the pipeline runs
    BwdFormIn K;
    K.n = 3; K.which[0] = 3; K.which[1] = 2; K.which[2] = 1; K.train[0] = 1; K.grids = true; K.N = 1000;
    BwdForm F = bwd_form(K);                               // the Mapper's colour stage: one trainable role beside two frozen ones
    if (F.kernel != BWD_MULTI || F.train_role != 0 || !F.skip_eligible || !F.deal_eligible || !F.scan_may_ride || F.waves != 8) { ++failures; fprintf(stderr, "FAIL form: colour stage\n"); }
    K.n = 2; K.which[0] = 2; K.which[1] = 1; K.train[0] = 0;
    F = bwd_form(K);                                       // its fine stage: the 16-wave kernel, which never deals
    if (F.kernel != BWD_FROZEN || F.train_role != -1 || !F.skip_eligible || F.deal_eligible || F.waves != 16 || F.scan_halves != 4) { ++failures; fprintf(stderr, "FAIL form: fine stage\n"); }
    K.n = 3; K.which[0] = 3; K.which[1] = 2; K.which[2] = 1; K.grids = false; K.rays = true; K.track = true; K.N = 200;
    F = bwd_form(K);                                       // the Tracker
    if (F.kernel != BWD_TRACK || !F.mask_ok || F.skip_eligible || F.scan_may_ride) { ++failures; fprintf(stderr, "FAIL form: Tracker\n"); }
    if (median_form(true, false, 0, 0, 200, 256, true, false, false) != MEDIAN_DEFERRED || median_form(true, false, 0, 1, 200, 256, true, false, false) != MEDIAN_BARRIER ||
        median_form(true, false, 0, 1, 1024, 256, true, false, false) != MEDIAN_BARRIER || median_form(true, false, 0, 1, 1025, 256, true, false, false) != MEDIAN_THREE ||
        median_form(true, false, 0, 1, 201, 50, true, false, false) != MEDIAN_THREE || median_form(true, false, 0, 1, 200, 50, true, false, false) != MEDIAN_BARRIER) {
        ++failures; fprintf(stderr, "FAIL form: median at its boundaries\n");
    }
    if (bwd_separate_grid(256, 3000, false) != 256 || bwd_separate_grid(256, 9, false) != 2 || bwd_separate_grid(256, 0, false) != 1 || bwd_separate_grid(256, 3000, true) != 1) {
        ++failures; fprintf(stderr, "FAIL form: bwd_separate_grid\n");
    }
    return forms;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "--dump")) return dump();
    if (argc != 2) { fprintf(stderr, "usage: split_test <table> | --dump\n"); return 2; }
    literal_cases();
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char line[256];
    long rows = 0;
    while (fgets(line, sizeof(line), f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        Row W, R;
        memset(&W, 0, sizeof(W));
        if (sscanf(line, "%c %d %d %d %d %d %d %d %d %d %d %d | %d %d %d %ld", &W.fn, &W.num_cu, &W.ntasks, &W.n, &W.waves, &W.train_role, &W.cost[0], &W.cost[1],
                   &W.cost[2], &W.tasks[0], &W.tasks[1], &W.tasks[2], &W.w[0], &W.w[1], &W.w[2], &W.makespan) != 16 ||
            !strchr("SBT", W.fn) || W.n < 1 || W.n > 3 || W.ntasks < 1 || W.waves < 1 || W.num_cu < 3 || (W.fn == 'T' && (W.train_role < 0 || W.train_role >= W.n))) {
            fprintf(stderr, "bad row: %s", line); fclose(f); return 2;
        }
        R = W;
        compute(R);
        ++rows;
        if (memcmp(R.w, W.w, sizeof(R.w)) != 0 || R.makespan != W.makespan) { if (++failures < 20) { fprintf(stderr, "FAIL table: want %sgot  ", line); print_row(stderr, R); } }
        else if (!within_caps(R)) { if (++failures < 20) { fprintf(stderr, "FAIL caps: "); print_row(stderr, R); } }
    }
    fclose(f);
    const int table_failures = failures;
    const long plans = knob_sweep();
    printf("split_test: knob sweep %ld plans, %d failures\n", plans, failures - table_failures);
    const int knob_failures = failures;
    const long forms = form_sweep();
    printf("split_test: form sweep %ld forms, %d failures\n", forms, failures - knob_failures);
    printf("split_test: %ld rows, %d failures\n", rows, failures);
    return failures ? 1 : 0;
}
