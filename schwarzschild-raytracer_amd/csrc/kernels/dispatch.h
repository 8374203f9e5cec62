// dispatch.h — which instantiations of geodesic.hip's kernel templates exist,
// which of them a launch runs, and which launches are refused: stated once.
// Host code without a HIP header (it builds with plain g++). geodesic.hip's
// launchers expand the lists and call the functions; tests/test_dispatch.py
// holds both to the rules on the CPU, because every instantiation computes
// the same pixels: a wrong selection shows in the frame time alone.
#ifndef SR_DISPATCH_H
#define SR_DISPATCH_H

#include <stddef.h>
#include <stdint.h>

#include "../device_scene.h"

// ---- the capacities the integrate kernel is instantiated for
// The small instantiation's budget slots (the default scene has six: phase 1
// of an event runs over every slot of the capacity) and budgeted cylinders
#ifndef SR_NB_SMALL
#define SR_NB_SMALL 6
#endif
#ifndef SR_NC_SMALL  // round 6: 0 (no budgeted cylinder needs the direction tests, precompute.cpp SR_CYL_DIRFREE)
#define SR_NC_SMALL 0
#endif
// Budgeted cylinders whose nearly parallel chords the kernel handles apart
// (chord_parallel, slab budgets, the cylinder-plane fast loops) in the
// general and large instantiations and the resume kernel: none since round 6;
// SR_MAX_CYLINDERS for a host built with SR_CYL_DIRFREE=0
#ifndef SR_NC_KERNEL
#define SR_NC_KERNEL 0
#endif
// the general instantiation: 8 slots; scenes with more run the large one
// (every object budgeted: SR_MAX_BUDGET slots)
#define SR_NB_GENERAL 8
#define SR_NC_GENERAL SR_NC_KERNEL
#ifndef SR_FAST_UNROLL  // fast-loop steps per iteration (1 .. 4; the step table has 4 padding entries);
                        // the latency mode's instantiation runs 2 (sr_set_latency_mode). 4 since round 6:
                        // at 7 waves per SIMD 0.5 % more frames per second than 3 in two A/Bs
                        // (profiles/r06/s18, s19), one frame alone level
#define SR_FAST_UNROLL SR_FAST_UNROLL_DEFAULT
#endif

// ---- the kinds: a kernel's template arguments, in the kernel's own order
struct sr_integrate_kind { bool cull, wcost; int nb, fu, nc; bool tr; int proj; bool seq; };
struct sr_shade_kind { bool sparse, seq; };
struct sr_resume_kind { bool cull, tr, seq; };
struct sr_trace_kind { bool cull, tr; };
inline bool operator==(const sr_integrate_kind& a, const sr_integrate_kind& b) {
    return a.cull == b.cull && a.wcost == b.wcost && a.nb == b.nb && a.fu == b.fu && a.nc == b.nc && a.tr == b.tr &&
           a.proj == b.proj && a.seq == b.seq;
}
inline bool operator==(const sr_shade_kind& a, const sr_shade_kind& b) { return a.sparse == b.sparse && a.seq == b.seq; }
inline bool operator==(const sr_resume_kind& a, const sr_resume_kind& b) { return a.cull == b.cull && a.tr == b.tr && a.seq == b.seq; }
inline bool operator==(const sr_trace_kind& a, const sr_trace_kind& b) { return a.cull == b.cull && a.tr == b.tr; }

// ---- the instantiated kinds: X(template arguments) per kernel the library
// holds (27 + 3 + 5 + 3); no other kind is built or can be launched. The
// lists' order, a frame launch's kinds (SEQ false) ahead of a sequence
// launch's, is the order of the kernels in the code object.
// An angular projection's four (sr.h "Projections"): wave costs, culling off,
// the small layout, all slots. The overlay is tested per chord (TR false) and
// the latency mode runs the default unroll, with the same pixels.
#define SR_INTEGRATE_KINDS_PROJECTED(X, P)                                         \
    X(true, true, SR_MAX_BUDGET, SR_FAST_UNROLL, SR_NC_KERNEL, false, P, false)    \
    X(false, false, 1, SR_FAST_UNROLL, 1, false, P, false)                         \
    X(true, false, SR_NB_SMALL, SR_FAST_UNROLL, SR_NC_SMALL, false, P, false)      \
    X(true, false, SR_MAX_BUDGET, SR_FAST_UNROLL, SR_NC_KERNEL, false, P, false)
// A sequence launch's three per projection (sr.h "Scene sequences"): culling
// off, the small layout (fr.num_budget and fr.num_budget_cyl are the window's
// maxima), all slots; the overlay and the latency mode as above
#define SR_INTEGRATE_KINDS_SEQ(X, P)                                               \
    X(false, false, 1, SR_FAST_UNROLL, 1, false, P, true)                          \
    X(true, false, SR_NB_SMALL, SR_FAST_UNROLL, SR_NC_SMALL, false, P, true)       \
    X(true, false, SR_MAX_BUDGET, SR_FAST_UNROLL, SR_NC_KERNEL, false, P, true)
// The pinhole's ten: wave costs (general, large); the test ray budgeted (small,
// general, large); the latency mode's unroll (small only); small, general,
// large; the reference's loop (no budgets: the smallest LDS layout)
#define SR_INTEGRATE_KINDS(X)                                                                                \
    SR_INTEGRATE_KINDS_PROJECTED(X, SR_PROJECTION_EQUIRECT)                                                  \
    SR_INTEGRATE_KINDS_PROJECTED(X, SR_PROJECTION_FISHEYE)                                                   \
    X(true, true, SR_NB_GENERAL, SR_FAST_UNROLL, SR_NC_GENERAL, false, SR_PROJECTION_RECTILINEAR, false)     \
    X(true, true, SR_MAX_BUDGET, SR_FAST_UNROLL, SR_NC_KERNEL, false, SR_PROJECTION_RECTILINEAR, false)      \
    X(true, false, SR_NB_SMALL, SR_FAST_UNROLL, SR_NC_SMALL, true, SR_PROJECTION_RECTILINEAR, false)         \
    X(true, false, SR_NB_GENERAL, SR_FAST_UNROLL, SR_NC_GENERAL, true, SR_PROJECTION_RECTILINEAR, false)     \
    X(true, false, SR_MAX_BUDGET, SR_FAST_UNROLL, SR_NC_KERNEL, true, SR_PROJECTION_RECTILINEAR, false)      \
    X(true, false, SR_NB_SMALL, 2, SR_NC_SMALL, false, SR_PROJECTION_RECTILINEAR, false)                     \
    X(true, false, SR_NB_SMALL, SR_FAST_UNROLL, SR_NC_SMALL, false, SR_PROJECTION_RECTILINEAR, false)        \
    X(true, false, SR_NB_GENERAL, SR_FAST_UNROLL, SR_NC_GENERAL, false, SR_PROJECTION_RECTILINEAR, false)    \
    X(true, false, SR_MAX_BUDGET, SR_FAST_UNROLL, SR_NC_KERNEL, false, SR_PROJECTION_RECTILINEAR, false)     \
    X(false, false, 1, SR_FAST_UNROLL, 1, false, SR_PROJECTION_RECTILINEAR, false)                           \
    SR_INTEGRATE_KINDS_SEQ(X, SR_PROJECTION_EQUIRECT)                                                        \
    SR_INTEGRATE_KINDS_SEQ(X, SR_PROJECTION_FISHEYE)                                                         \
    SR_INTEGRATE_KINDS_SEQ(X, SR_PROJECTION_RECTILINEAR)
#define SR_SHADE_KINDS(X) X(true, false) X(false, false) X(false, true)
#define SR_RESUME_KINDS(X) X(true, true, false) X(true, false, false) X(false, false, false) X(true, false, true) X(false, false, true)
#define SR_TRACE_KINDS(X) X(true, true) X(true, false) X(false, false)

// ---- the selection
// the small layout fits the scene
inline bool sr_kind_small(const sr_dev_frame& fr) {
    return fr.cull != 0 && fr.num_budget <= SR_NB_SMALL && fr.num_budget_cyl <= SR_NC_SMALL;
}
// the test ray is budgeted (clearance_tr) instead of tested per chord
inline bool sr_kind_tr(const sr_dev_frame& fr) { return fr.cull != 0 && fr.tr_visible != 0; }

// The integrate kernel of a frame launch (sparse or not) or a sequence launch:
// the layout that holds the scene, then at most one variant of it. The wave
// costs win over the overlay (and always cull), the overlay over the latency
// mode's unroll; only the pinhole's frame launch has the general layout, the
// test ray budgeted and the 2-step unroll.
inline sr_integrate_kind sr_select_integrate(const sr_dev_frame& fr, bool seq) {
    const bool cull = fr.cull != 0, small = sr_kind_small(fr);
    const bool pinhole = !seq && fr.projection == SR_PROJECTION_RECTILINEAR, general = pinhole && fr.num_budget <= SR_NB_GENERAL;
    const sr_integrate_kind none{false, false, 1, SR_FAST_UNROLL, 1, false, fr.projection, seq};
    const sr_integrate_kind sm{true, false, SR_NB_SMALL, SR_FAST_UNROLL, SR_NC_SMALL, false, fr.projection, seq};
    const sr_integrate_kind gen{true, false, SR_NB_GENERAL, SR_FAST_UNROLL, SR_NC_GENERAL, false, fr.projection, seq};
    const sr_integrate_kind all{true, false, SR_MAX_BUDGET, SR_FAST_UNROLL, SR_NC_KERNEL, false, fr.projection, seq};
    sr_integrate_kind k = !cull ? none : small ? sm : general ? gen : all;
    if (fr.wave_cost && !seq) {
        k = general ? gen : all;
        k.wcost = true;
    } else if (pinhole && sr_kind_tr(fr)) {
        k.tr = true;
    } else if (pinhole && small && fr.fast_unroll == 2) {
        k.fu = 2;
    }
    return k;
}
// The shade kernel: a sparse launch reads its tiles from the list of codes, a sequence launch its scene per frame
inline sr_shade_kind sr_select_shade(bool seq, bool sparse) { return sr_shade_kind{sparse, !sparse && seq}; }
// The resume kernel of a frame launch or a reshade (the test ray budgeted, by
// the frame and not by the integrate kind: a projected launch with the overlay
// visible resumes with it budgeted), or of a sequence launch (never budgeted)
inline sr_resume_kind sr_select_resume(const sr_dev_frame& fr, bool seq) {
    return sr_resume_kind{fr.cull != 0, !seq && sr_kind_tr(fr), seq};
}
// The trace kernel: the resume kernel's rule
inline sr_trace_kind sr_select_trace(const sr_dev_frame& fr) { return sr_trace_kind{fr.cull != 0, sr_kind_tr(fr)}; }

// ---- the checks: what a launcher refuses (hipErrorInvalidValue) before it
// records an event or launches anything
enum sr_launch_type { SR_LAUNCH_FRAME, SR_LAUNCH_SEQ, SR_LAUNCH_RESHADE };
enum sr_verdict { SR_LAUNCH_REJECT, SR_LAUNCH_EMPTY /* nothing to do: hipSuccess */, SR_LAUNCH_GO };
// what the checks read of a launch besides its frame
struct sr_launch_ptrs { const void *sc, *xtab, *ps, *list, *count, *order, *cost, *diag, *start; size_t ps_n; };
struct sr_launch_plan {
    sr_verdict verdict;
    // order without cost (sr_render_adaptive): one frame, of which only the tiles whose codes `order` lists are
    // integrated and shaded (-1 behind them); no cost is recorded, no order computed, split tiles do not apply
    bool sparse;
    int split, split_log2;  // split tiles (they need the launch order: their codes come from order_tiles); 0, 6 without
    unsigned gx, gy, tiles;  // the frame's grid of 16x16 tiles
    unsigned slots;  // the integrate grid's launch codes per frame: the tiles and the split tiles' further workgroups
};

inline sr_launch_plan sr_plan_launch(sr_launch_type type, const sr_dev_frame& fr, const sr_launch_ptrs& a) {
    const unsigned gx = (unsigned)((fr.width + 15) / 16), gy = (unsigned)((fr.nrows + 15) / 16);
    sr_launch_plan p{gx && gy ? SR_LAUNCH_REJECT : SR_LAUNCH_EMPTY, false, 0, 6, gx, gy, gx * gy, 0};
    if (p.verdict == SR_LAUNCH_EMPTY) return p;
    const unsigned B = (unsigned)fr.batch;
    if (B < 1 || B > SR_MAX_BATCH || fr.tiles != (int)p.tiles) return p;
    if ((size_t)p.tiles * B * 256 > a.ps_n || (size_t)p.tiles * B * 256 > (size_t)INT32_MAX) return p;
    if (p.tiles > (1u << 22)) return p;  // tile << 8 stays a positive int
    if (fr.projection < SR_PROJECTION_RECTILINEAR || fr.projection > SR_PROJECTION_FISHEYE) return p;
    // cylinders with direction tests beyond what the instantiations handle (a
    // host built with SR_CYL_DIRFREE=0 against a kernel without them)
    if (fr.cull != 0 && fr.num_budget_cyl > SR_NC_KERNEL && !sr_kind_small(fr)) return p;
    if (type == SR_LAUNCH_FRAME) {
        if (!a.start || (a.cost && !a.order)) return p;
        p.sparse = a.order && !a.cost;
        if (p.sparse && (B != 1 || fr.wave_cost)) return p;
    } else if (type == SR_LAUNCH_SEQ) {
        if (!a.start || !a.sc || !a.xtab || (a.cost == nullptr) != (a.order == nullptr) || fr.wave_cost) return p;
    } else if (!a.ps || !a.list || !a.count || !a.diag || fr.wave_cost) {  // a reshade
        return p;
    }
    p.split = a.order && !p.sparse ? fr.split_tiles : 0;
    if (p.split < 0 || (p.split && (fr.split_log2 < 0 || fr.split_log2 > 4 || (fr.split_log2 & 1)))) return p;
    if (p.split) p.split_log2 = fr.split_log2;
    p.slots = p.tiles + ((64u >> p.split_log2) - 1u) * (unsigned)p.split;
    p.verdict = SR_LAUNCH_GO;
    return p;
}

// sr_launch_trace's: the rays, at least one output, and the cylinders the trace kernel's layout (the resume kernel's) holds
inline sr_verdict sr_check_trace(const sr_dev_frame* fr, int n_rays, bool inputs, bool any_output) {
    if (n_rays < 0 || n_rays > SR_TRACE_MAX_RAYS) return SR_LAUNCH_REJECT;
    if (n_rays == 0) return SR_LAUNCH_EMPTY;
    if (!fr || !inputs || !any_output || (fr->cull != 0 && fr->num_budget_cyl > SR_NC_KERNEL)) return SR_LAUNCH_REJECT;
    return SR_LAUNCH_GO;
}

#endif
