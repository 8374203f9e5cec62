// The launch dispatch of csrc/kernels/dispatch.h against its rules, written
// out here row by row with the default capacities as numbers (6, 8 and 21
// slots, no budgeted cylinders, 4 steps per fast-loop iteration), over the
// whole product of what the selection reads. Host code only: it links nothing
// and needs no GPU. Prints the table of instantiated kinds as the demangled
// kernel names (tests/test_dispatch.py compares them with the libraries'
// symbols), then "ALL OK".
#include <cstdio>
#include <string>
#include <vector>

#include "device_scene.h"
#include "kernels/dispatch.h"

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            failures++;                                    \
            std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
        }                                                  \
    } while (0)

static const char* tf(bool b) { return b ? "true" : "false"; }
static std::string name(const sr_integrate_kind& k) {
    char s[160];
    std::snprintf(s, sizeof s, "sr_integrate_kernel<%s, %s, %d, %d, %d, %s, %d, %s>", tf(k.cull), tf(k.wcost), k.nb, k.fu,
                  k.nc, tf(k.tr), k.proj, tf(k.seq));
    return s;
}
static std::string name(const sr_shade_kind& k) {
    return std::string("sr_shade_kernel<") + tf(k.sparse) + ", " + tf(k.seq) + ">";
}
static std::string name(const sr_resume_kind& k) {
    return std::string("sr_resume_kernel<") + tf(k.cull) + ", " + tf(k.tr) + ", " + tf(k.seq) + ">";
}
static std::string name(const sr_trace_kind& k) { return std::string("sr_trace_kernel<") + tf(k.cull) + ", " + tf(k.tr) + ">"; }

// a family's table, and how often the product selected each of its kinds
template <class K>
struct Table {
    std::vector<K> kinds;
    std::vector<long> selected;
    void select(const K& k, const char* what) {
        for (size_t i = 0; i < kinds.size(); i++)
            if (kinds[i] == k) {
                selected[i]++;
                return;
            }
        CHECK(false, "%s selects %s, which is not in the table", what, name(k).c_str());
    }
    void finish(size_t count) {
        CHECK(kinds.size() == count, "%zu kinds, %zu expected", kinds.size(), count);
        for (size_t i = 0; i < kinds.size(); i++) {
            std::printf("%s\n", name(kinds[i]).c_str());
            CHECK(selected[i] > 0, "%s is in the table and no accepted launch of the product selects it", name(kinds[i]).c_str());
            for (size_t j = 0; j < i; j++) CHECK(!(kinds[i] == kinds[j]), "%s is listed twice", name(kinds[i]).c_str());
        }
    }
};
#define SR_X(...) sr_integrate_kind{__VA_ARGS__},
static Table<sr_integrate_kind> integrate_table{{SR_INTEGRATE_KINDS(SR_X)}, {}};
#undef SR_X
#define SR_X(...) sr_shade_kind{__VA_ARGS__},
static Table<sr_shade_kind> shade_table{{SR_SHADE_KINDS(SR_X)}, {}};
#undef SR_X
#define SR_X(...) sr_resume_kind{__VA_ARGS__},
static Table<sr_resume_kind> resume_table{{SR_RESUME_KINDS(SR_X)}, {}};
#undef SR_X
#define SR_X(...) sr_trace_kind{__VA_ARGS__},
static Table<sr_trace_kind> trace_table{{SR_TRACE_KINDS(SR_X)}, {}};
#undef SR_X

// ---- the rules, as rows. A row: {cull, wcost, nb, fu, nc, tr, proj, seq}

static sr_integrate_kind expect_integrate(bool cull, int nb, int nbc, bool trv, int fu, int proj, bool wc, bool seq) {
    const bool small = cull && nb <= 6 && nbc <= 0, general = nb <= 8, tr = cull && trv;
    if (seq) {  // three per projection
        if (!cull) return {false, false, 1, 4, 1, false, proj, true};
        if (small) return {true, false, 6, 4, 0, false, proj, true};
        return {true, false, 21, 4, 0, false, proj, true};
    }
    if (proj != 0) {  // equirect, fisheye: four per projection
        if (wc) return {true, true, 21, 4, 0, false, proj, false};
        if (!cull) return {false, false, 1, 4, 1, false, proj, false};
        if (small) return {true, false, 6, 4, 0, false, proj, false};
        return {true, false, 21, 4, 0, false, proj, false};
    }
    if (wc && general) return {true, true, 8, 4, 0, false, 0, false};            //  1
    if (wc) return {true, true, 21, 4, 0, false, 0, false};                      //  2
    if (small && tr) return {true, false, 6, 4, 0, true, 0, false};              //  3
    if (cull && general && tr) return {true, false, 8, 4, 0, true, 0, false};    //  4
    if (cull && tr) return {true, false, 21, 4, 0, true, 0, false};              //  5
    if (small && fu == 2) return {true, false, 6, 2, 0, false, 0, false};        //  6
    if (small) return {true, false, 6, 4, 0, false, 0, false};                   //  7
    if (cull && general) return {true, false, 8, 4, 0, false, 0, false};         //  8
    if (cull) return {true, false, 21, 4, 0, false, 0, false};                   //  9
    return {false, false, 1, 4, 1, false, 0, false};                             // 10
}
static sr_resume_kind expect_resume(bool cull, bool trv, bool seq) {
    if (seq) return {cull, false, true};
    if (cull && trv) return {true, true, false};
    if (cull) return {true, false, false};
    return {false, false, false};
}
static sr_shade_kind expect_shade(bool sparse, bool seq) {
    if (sparse) return {true, false};
    if (seq) return {false, true};
    return {false, false};
}
static sr_trace_kind expect_trace(bool cull, bool trv) {
    if (cull && trv) return {true, true};
    if (cull) return {true, false};
    return {false, false};
}

// ---- a valid launch of each type: 68 x 44 pixels, 5 x 3 tiles

enum Launch { FRAME, SPARSE, SEQUENCE, RESHADE, TRACE, LAUNCHES };
static const char* const launch_names[LAUNCHES] = {"frame", "sparse", "sequence", "reshade", "trace"};
static int dummy;

static sr_dev_frame frame_of(int batch) {
    static sr_dev_frame fr;  // 9 KiB of zeros
    fr = sr_dev_frame{};
    fr.width = 68;
    fr.nrows = fr.height = 44;
    fr.tiles = 15;
    fr.batch = batch;
    fr.max_steps = 400;
    fr.cull = 1;
    fr.num_budget = 6;
    fr.fast_unroll = 4;
    fr.projection = SR_PROJECTION_RECTILINEAR;
    return fr;
}
static sr_launch_ptrs ptrs_of(Launch l, const sr_dev_frame& fr) {
    const void* const p = &dummy;
    sr_launch_ptrs a{p, nullptr, p, p, p, nullptr, nullptr, p, p, (size_t)fr.tiles * fr.batch * 256};
    if (l == FRAME || l == SEQUENCE) a.order = a.cost = p;
    if (l == SPARSE) a.order = p;
    if (l == SEQUENCE) a.xtab = p;
    if (l == RESHADE) a.start = nullptr;
    return a;
}
static sr_launch_type type_of(Launch l) {
    return l == SEQUENCE ? SR_LAUNCH_SEQ : l == RESHADE ? SR_LAUNCH_RESHADE : SR_LAUNCH_FRAME;
}
static sr_verdict verdict(Launch l, const sr_dev_frame& fr, const sr_launch_ptrs& a) {
    return sr_plan_launch(type_of(l), fr, a).verdict;
}

// ---- 1, 2, 3: the product

static void product() {
    integrate_table.selected.assign(integrate_table.kinds.size(), 0);
    shade_table.selected.assign(shade_table.kinds.size(), 0);
    resume_table.selected.assign(resume_table.kinds.size(), 0);
    trace_table.selected.assign(trace_table.kinds.size(), 0);
    const int budgets[] = {0, 1, 6, 7, 8, 9, 21};
    long cases = 0, accepted = 0;
    for (int cull = 0; cull < 2; cull++)
    for (int nb : budgets)
    for (int nbc = 0; nbc < 2; nbc++)
    for (int trv = 0; trv < 2; trv++)
    for (int fu = 2; fu <= 4; fu += 2)
    for (int proj = 0; proj < 3; proj++)
    for (int wc = 0; wc < 2; wc++)
    for (int li = 0; li < LAUNCHES; li++) {
        const Launch l = (Launch)li;
        sr_dev_frame fr = frame_of(l == SPARSE ? 1 : 3);
        fr.cull = cull;
        fr.num_budget = nb;
        fr.num_budget_cyl = nbc;
        fr.tr_visible = trv;
        fr.fast_unroll = fu;
        fr.projection = proj;
        fr.wave_cost = wc ? &dummy : nullptr;
        char what[160];
        std::snprintf(what, sizeof what, "%s cull %d num_budget %d num_budget_cyl %d tr_visible %d fast_unroll %d projection %d wave_cost %d",
                      launch_names[l], cull, nb, nbc, trv, fu, proj, wc);
        cases++;
        // the rejection list: a budgeted cylinder with direction tests is beyond
        // every layout (the small one holds none either); wave costs are a plain
        // frame launch's alone (a trace launch does not read them)
        const bool beyond = cull && nbc > 0;
        const bool expect_go = !beyond && !(wc && (l == SPARSE || l == SEQUENCE || l == RESHADE));
        const bool seq = l == SEQUENCE;
        if (l == TRACE) {
            const sr_verdict v = sr_check_trace(&fr, 1000, true, true);
            CHECK((v == SR_LAUNCH_GO) == expect_go, "%s: verdict %d", what, (int)v);
            CHECK(v != SR_LAUNCH_EMPTY, "%s", what);
            const sr_trace_kind k = sr_select_trace(fr);
            CHECK(k == expect_trace(cull, trv), "%s: %s", what, name(k).c_str());
            CHECK(!cull || nbc <= SR_NC_KERNEL || v == SR_LAUNCH_REJECT, "%s: a cylinder beyond the trace kernel's layout", what);
            if (v == SR_LAUNCH_GO) trace_table.select(k, what), accepted++;
            continue;
        }
        const sr_launch_plan p = sr_plan_launch(type_of(l), fr, ptrs_of(l, fr));
        CHECK((p.verdict == SR_LAUNCH_GO) == expect_go, "%s: verdict %d", what, (int)p.verdict);
        CHECK(p.verdict != SR_LAUNCH_EMPTY, "%s", what);
        CHECK(p.sparse == (l == SPARSE) || p.verdict != SR_LAUNCH_GO, "%s: sparse %d", what, (int)p.sparse);
        const sr_integrate_kind ik = sr_select_integrate(fr, seq);
        const sr_shade_kind sk = sr_select_shade(seq, l == SPARSE);
        const sr_resume_kind rk = sr_select_resume(fr, seq);
        if (l != RESHADE) {
            CHECK(ik == expect_integrate(cull, nb, nbc, trv, fu, proj, wc, seq), "%s: %s", what, name(ik).c_str());
            // 2. sound: the layout holds the scene, or the launch is refused
            if (cull) {
                CHECK(ik.cull && ik.nb >= nb, "%s: %s holds too few slots", what, name(ik).c_str());
                CHECK(ik.nc >= nbc || p.verdict == SR_LAUNCH_REJECT, "%s: %s holds too few cylinders", what, name(ik).c_str());
            }
            if (p.verdict == SR_LAUNCH_GO) CHECK(ik.wcost == (wc != 0), "%s: %s", what, name(ik).c_str());
        }
        CHECK(sk == expect_shade(l == SPARSE, seq), "%s: %s", what, name(sk).c_str());
        CHECK(rk == expect_resume(cull, trv, seq), "%s: %s", what, name(rk).c_str());
        CHECK(!cull || nbc <= SR_NC_KERNEL || p.verdict == SR_LAUNCH_REJECT, "%s: a cylinder beyond the resume kernel's layout", what);
        if (p.verdict == SR_LAUNCH_GO) {  // 3. what is launched is in the table
            accepted++;
            if (l != RESHADE) integrate_table.select(ik, what);
            shade_table.select(sk, what);
            resume_table.select(rk, what);
        }
    }
    CHECK(cases == 2 * 7 * 2 * 2 * 2 * 3 * 2 * 5, "%ld cases", cases);
    CHECK(accepted > cases / 4, "%ld of %ld accepted", accepted, cases);
}

// ---- 1: the precedence cases, by name

static sr_dev_frame scene_frame(int nb, bool trv, int fu, int proj, bool wc) {
    sr_dev_frame fr = frame_of(1);
    fr.num_budget = nb;
    fr.tr_visible = trv;
    fr.fast_unroll = fu;
    fr.projection = proj;
    fr.wave_cost = wc ? &dummy : nullptr;
    return fr;
}
static void precedence() {
    // the overlay over the latency unroll
    CHECK((sr_select_integrate(scene_frame(6, true, 2, 0, false), false) == sr_integrate_kind{true, false, 6, 4, 0, true, 0, false}), "overlay over unroll");
    // the wave cost over the overlay, and over the unroll
    CHECK((sr_select_integrate(scene_frame(6, true, 2, 0, true), false) == sr_integrate_kind{true, true, 8, 4, 0, false, 0, false}), "wave cost over overlay");
    CHECK((sr_select_integrate(scene_frame(9, true, 4, 0, true), false) == sr_integrate_kind{true, true, 21, 4, 0, false, 0, false}), "wave cost over overlay, large");
    // in the wave-cost launch the general layout does not ask for culling
    sr_dev_frame off = scene_frame(6, false, 4, 0, true);
    off.cull = 0;
    CHECK((sr_select_integrate(off, false) == sr_integrate_kind{true, true, 8, 4, 0, false, 0, false}), "wave cost, culling off");
    // a projected launch with the overlay visible: per chord in the integrate kernel, budgeted in the resume kernel
    for (int proj = 1; proj <= 2; proj++) {
        const sr_dev_frame fr = scene_frame(6, true, 2, proj, false);
        CHECK((sr_select_integrate(fr, false) == sr_integrate_kind{true, false, 6, 4, 0, false, proj, false}), "projection %d", proj);
        CHECK((sr_select_resume(fr, false) == sr_resume_kind{true, true, false}), "projection %d", proj);
    }
    // a sequence launch with the overlay visible: no TR anywhere
    for (int proj = 0; proj <= 2; proj++) {
        const sr_dev_frame fr = scene_frame(7, true, 2, proj, false);
        CHECK((sr_select_integrate(fr, true) == sr_integrate_kind{true, false, 21, 4, 0, false, proj, true}), "projection %d", proj);
        CHECK((sr_select_resume(fr, true) == sr_resume_kind{true, false, true}), "projection %d", proj);
        CHECK((sr_select_shade(true, false) == sr_shade_kind{false, true}), "projection %d", proj);
    }
    // 6 slots: small; 7 and 8: general; 9 and 21: large
    const int nbs[] = {6, 7, 8, 9, 21}, layout[] = {6, 8, 8, 21, 21};
    for (int i = 0; i < 5; i++)
        for (int trv = 0; trv < 2; trv++)
            CHECK((sr_select_integrate(scene_frame(nbs[i], trv, 4, 0, false), false) ==
                   sr_integrate_kind{true, false, layout[i], 4, 0, trv != 0, 0, false}), "num_budget %d overlay %d", nbs[i], trv);
    // the latency unroll: the small layout's alone
    CHECK((sr_select_integrate(scene_frame(6, false, 2, 0, false), false) == sr_integrate_kind{true, false, 6, 2, 0, false, 0, false}), "unroll");
    CHECK((sr_select_integrate(scene_frame(7, false, 2, 0, false), false) == sr_integrate_kind{true, false, 8, 4, 0, false, 0, false}), "unroll, general");
}

// ---- the rejection list, one argument at a time on launches that are
// accepted without it

static void rejections() {
    for (int li = 0; li < TRACE; li++) {
        const Launch l = (Launch)li;
        const char* const n = launch_names[l];
        const int B = l == SPARSE ? 1 : 3;
        const sr_dev_frame ok = frame_of(B);
        const sr_launch_ptrs a = ptrs_of(l, ok);
        CHECK(verdict(l, ok, a) == SR_LAUNCH_GO, "%s", n);
        sr_dev_frame fr;
        sr_launch_ptrs b;
        // an empty grid is no error, whatever else is wrong
        fr = ok, fr.width = 0, fr.batch = 0;
        CHECK(verdict(l, fr, a) == SR_LAUNCH_EMPTY, "%s", n);
        fr = ok, fr.nrows = 0, fr.projection = 7;
        CHECK(verdict(l, fr, a) == SR_LAUNCH_EMPTY, "%s", n);
        // batch outside 1 .. SR_MAX_BATCH
        for (int batch : {0, -1, SR_MAX_BATCH + 1}) {
            fr = ok, fr.batch = batch;
            b = a, b.ps_n = (size_t)1 << 30;
            CHECK(verdict(l, fr, b) == SR_LAUNCH_REJECT, "%s batch %d", n, batch);
        }
        if (l != SPARSE) {
            fr = ok, fr.batch = SR_MAX_BATCH;
            b = a, b.ps_n = (size_t)15 * SR_MAX_BATCH * 256;
            CHECK(verdict(l, fr, b) == SR_LAUNCH_GO, "%s batch %d", n, SR_MAX_BATCH);
        }
        // tiles != grid.x * grid.y
        fr = ok, fr.tiles = 14;
        CHECK(verdict(l, fr, a) == SR_LAUNCH_REJECT, "%s tiles", n);
        fr = ok, fr.width = 81;
        CHECK(verdict(l, fr, a) == SR_LAUNCH_REJECT, "%s tiles", n);
        // the pixel state's capacity
        b = a, b.ps_n--;
        CHECK(verdict(l, ok, b) == SR_LAUNCH_REJECT, "%s ps_n", n);
        // 2^22 tiles are the most; 2^31 pixel ids are too many
        b = a, b.ps_n = (size_t)1 << 40;
        fr = frame_of(1), fr.width = fr.nrows = 16 * 2048, fr.tiles = 1 << 22;
        CHECK(verdict(l, fr, b) == SR_LAUNCH_GO, "%s 2^22 tiles", n);
        fr.batch = 2;
        CHECK(verdict(l, fr, b) == SR_LAUNCH_REJECT, "%s 2^31 ids", n);
        fr = frame_of(1), fr.width = 16 * 2049, fr.nrows = 16 * 2048, fr.tiles = 2049 * 2048;
        CHECK(verdict(l, fr, b) == SR_LAUNCH_REJECT, "%s over 2^22 tiles", n);
        // the projection
        for (int proj : {-1, 3}) {
            fr = ok, fr.projection = proj;
            CHECK(verdict(l, fr, a) == SR_LAUNCH_REJECT, "%s projection %d", n, proj);
        }
        // wave costs: the plain frame launch's alone
        fr = ok, fr.wave_cost = &dummy;
        CHECK(verdict(l, fr, a) == (l == FRAME ? SR_LAUNCH_GO : SR_LAUNCH_REJECT), "%s wave_cost", n);
        // split tiles: with a launch order that is no sparse list
        const bool splits = l == FRAME || l == SEQUENCE;
        for (int lg : {-2, 0, 1, 2, 3, 4, 5, 6}) {
            fr = ok, fr.split_tiles = 3, fr.split_log2 = lg;
            const bool good = lg == 0 || lg == 2 || lg == 4;
            const sr_launch_plan p = sr_plan_launch(type_of(l), fr, a);
            CHECK(p.verdict == (good || !splits ? SR_LAUNCH_GO : SR_LAUNCH_REJECT), "%s split_log2 %d", n, lg);
            if (p.verdict == SR_LAUNCH_GO) {
                CHECK(p.split == (splits ? 3 : 0) && p.split_log2 == (splits ? lg : 6), "%s split_log2 %d", n, lg);
                CHECK(p.slots == 15u + (splits ? ((64u >> lg) - 1u) * 3u : 0u), "%s split_log2 %d: %u slots", n, lg, p.slots);
                CHECK(p.gx == 5 && p.gy == 3 && p.tiles == 15, "%s grid", n);
            }
            b = a, b.order = b.cost = nullptr;  // no order: no split tiles
            if (l == FRAME) CHECK(sr_plan_launch(type_of(l), fr, b).split == 0 && verdict(l, fr, b) == SR_LAUNCH_GO, "%s", n);
        }
        fr = ok, fr.split_tiles = -1, fr.split_log2 = 2;
        CHECK(verdict(l, fr, a) == (splits ? SR_LAUNCH_REJECT : SR_LAUNCH_GO), "%s split_tiles -1", n);
        // the pointers
        if (l != RESHADE) {
            b = a, b.start = nullptr;
            CHECK(verdict(l, ok, b) == SR_LAUNCH_REJECT, "%s start", n);
        }
    }
    const sr_dev_frame f3 = frame_of(3), f1 = frame_of(1);
    sr_launch_ptrs b;
    // a frame launch: cost without order; order alone is a sparse launch, of one frame
    b = ptrs_of(FRAME, f3), b.order = nullptr;
    CHECK(verdict(FRAME, f3, b) == SR_LAUNCH_REJECT, "cost without order");
    b = ptrs_of(FRAME, f3), b.order = b.cost = nullptr;
    CHECK(verdict(FRAME, f3, b) == SR_LAUNCH_GO, "neither");
    CHECK(verdict(SPARSE, f3, ptrs_of(SPARSE, f3)) == SR_LAUNCH_REJECT, "sparse batch 3");
    CHECK(sr_plan_launch(SR_LAUNCH_FRAME, f1, ptrs_of(SPARSE, f1)).sparse, "sparse");
    CHECK(!sr_plan_launch(SR_LAUNCH_FRAME, f1, ptrs_of(FRAME, f1)).sparse, "not sparse");
    // a sequence launch: cost and order both or neither; the scenes and their table
    b = ptrs_of(SEQUENCE, f3), b.cost = nullptr;
    CHECK(verdict(SEQUENCE, f3, b) == SR_LAUNCH_REJECT, "sequence order alone");
    b = ptrs_of(SEQUENCE, f3), b.order = nullptr;
    CHECK(verdict(SEQUENCE, f3, b) == SR_LAUNCH_REJECT, "sequence cost alone");
    b = ptrs_of(SEQUENCE, f3), b.order = b.cost = nullptr;
    CHECK(verdict(SEQUENCE, f3, b) == SR_LAUNCH_GO, "sequence neither");
    b = ptrs_of(SEQUENCE, f3), b.sc = nullptr;
    CHECK(verdict(SEQUENCE, f3, b) == SR_LAUNCH_REJECT, "sequence sc");
    b = ptrs_of(SEQUENCE, f3), b.xtab = nullptr;
    CHECK(verdict(SEQUENCE, f3, b) == SR_LAUNCH_REJECT, "sequence xtab");
    // a reshade: the pixel state and the queue
    for (int k = 0; k < 4; k++) {
        b = ptrs_of(RESHADE, f3);
        (k == 0 ? b.ps : k == 1 ? b.list : k == 2 ? b.count : b.diag) = nullptr;
        CHECK(verdict(RESHADE, f3, b) == SR_LAUNCH_REJECT, "reshade pointer %d", k);
    }
    // a trace launch
    CHECK(sr_check_trace(&f1, -1, true, true) == SR_LAUNCH_REJECT, "n_rays -1");
    CHECK(sr_check_trace(&f1, SR_TRACE_MAX_RAYS, true, true) == SR_LAUNCH_GO, "n_rays max");
    CHECK(sr_check_trace(nullptr, SR_TRACE_MAX_RAYS + 1, true, true) == SR_LAUNCH_REJECT, "n_rays over");
    CHECK(sr_check_trace(nullptr, 0, false, false) == SR_LAUNCH_EMPTY, "no rays");
    CHECK(sr_check_trace(nullptr, 1, true, true) == SR_LAUNCH_REJECT, "no frame");
    CHECK(sr_check_trace(&f1, 1, false, true) == SR_LAUNCH_REJECT, "no inputs");
    CHECK(sr_check_trace(&f1, 1, true, false) == SR_LAUNCH_REJECT, "no outputs");
}

int main() {
    // the rows above are the default capacities'
    static_assert(SR_NB_SMALL == 6 && SR_NC_SMALL == 0 && SR_NB_GENERAL == 8 && SR_NC_GENERAL == 0 && SR_NC_KERNEL == 0 &&
                      SR_MAX_BUDGET == 21 && SR_FAST_UNROLL == 4,
                  "build this test without capacity overrides");
    product();
    precedence();
    rejections();
    integrate_table.finish(27);
    resume_table.finish(5);
    shade_table.finish(3);
    trace_table.finish(3);
    if (failures) {
        std::printf("%d FAILED\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
