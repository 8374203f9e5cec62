// uniform.h - the wave-uniformity the integrate and shade kernels assert
// (geodesic.hip, included inside its unnamed namespace), checked at run time
// in the SR_CHECK_UNIFORM build (lib/libsr_chk.so, tests/test_gpu_uniformity.py).
//
// The kernels say "this value is the same in every active lane" in three
// ways, none of which the compiler verifies: an "s" (SGPR) constraint of an
// asm statement (SR_PIN, the texture-size pins, the fast loops' "; keep"
// statements) and __builtin_amdgcn_readfirstlane used as an assertion. Given
// a per-lane operand the compiler satisfies either by taking the first active
// lane's value, silently. Every such place is a *site*, named in SR_USITES
// below, and goes through one of
//   SR_PIN(site, x)    asm volatile("" : "+s"(x))
//   SR_PIN6(s0, a, ..) six operands through one "+s" statement
//   SR_KEEP(site, x)   asm volatile("; keep %0" ::"s"(x))
//   SR_RFL(site, x)    __builtin_amdgcn_readfirstlane(x)
// which without SR_CHECK_UNIFORM expand to that text and nothing else (the
// shipping kernels' instructions do not change: DESIGN.md §7). With it each
// first compares the operand's 32 bits with the first active lane's over the
// active lanes (bits, not floats: the extreme tables put NaN into these
// fields), *before* the constraint or readfirstlane makes the value trivially
// uniform, and counts per site the waves that reached it (seen) and the waves
// whose lanes disagreed (bad). It only counts, with one lane's atomicAdd: no
// trap, no early exit, the kernel goes on as the shipping one would, and the
// test fails afterwards from the counters.
//
// A waterfall's head (`first = readfirstlane(key)` in shade and hit_opacity)
// selects lanes and asserts nothing: it is no site. The sites inside a
// waterfall are checked under its `key == first` mask, which is what the
// code relies on.
#ifndef SR_UNIFORM_H
#define SR_UNIFORM_H

#ifdef SR_CHECK_UNIFORM

// One name per textual occurrence, in source order.
#define SR_USITES(X)                                                                                              \
    /* pin_slot: a budget slot's record */                                                                        \
    X(SLOT_TYPE) X(SLOT_RB) X(SLOT_MP) X(SLOT_BR) X(SLOT_MU) X(SLOT_PL1) X(SLOT_QK)                               \
    X(SLOT_BC0) X(SLOT_BC1) X(SLOT_BC2) X(SLOT_X0) X(SLOT_POS0) X(SLOT_POS1) X(SLOT_POS2) X(SLOT_X1)              \
    X(SLOT_A00) X(SLOT_A01) X(SLOT_A02) X(SLOT_X2) X(SLOT_A10) X(SLOT_A11) X(SLOT_A12)                            \
    X(SLOT_A20) X(SLOT_A21) X(SLOT_A22)                                                                           \
    /* pin_start_slot: a frame's start record, per slot */                                                        \
    X(START_E) X(START_K2R) X(START_NEED) X(START_FLAGS) X(START_BC0) X(START_BC1) X(START_BC2)                   \
    X(START_XNEED) X(START_WN0) X(START_WN1) X(START_WN2) X(START_XPERI)                                          \
    /* budget_start: the start record's header */                                                                 \
    X(HEAD_E0) X(HEAD_E1) X(HEAD_UH0) X(HEAD_UH1) X(HEAD_KAP) X(HEAD_A2S) X(HEAD_CAP) X(HEAD_BH_OUT)              \
    X(HEAD_TR0) X(HEAD_TR1)                                                                                       \
    /* budget_event */                                                                                            \
    X(EVENT_SPENT)                                                                                                \
    /* shade_hit, under shade's waterfall */                                                                      \
    X(SHADE_SLOT) X(SHADE_FACE)                                                                                   \
    /* hit_opacity_uniform's texture sizes; hit_opacity's waterfall */                                            \
    X(OPQ_TSX) X(OPQ_TSY) X(OPQ_MSX) X(OPQ_MSY) X(OPQ_AW) X(OPQ_AH)                                               \
    X(OPQ_SLOT) X(OPQ_FACE)                                                                                       \
    /* integrate: a recording launch's step index, the fast and coasting loops' table entries */                  \
    X(STEP_I) X(FAST_KEEP) X(COAST_KEEP)                                                                          \
    /* sr_resume_kernel<SEQ>: the per-frame pass's scene index */                                                 \
    X(RESUME_FRAME)                                                                                               \
    /* sr_uniform_selftest_kernel only */                                                                         \
    X(SELF_LANE) X(SELF_CONST) X(SELF_NAN) X(SELF_BRANCH)

enum {
#define SR_USITE_ENUM(n) SR_U_##n,
    SR_USITES(SR_USITE_ENUM)
#undef SR_USITE_ENUM
        SR_U_NSITES
};

// [0] seen, [1] bad: waves per site. line: the site's source line, stored by
// the site itself (0 until a wave reaches it; the names need no run).
__device__ unsigned sr_u_count[2][SR_U_NSITES];
__device__ int sr_u_line[SR_U_NSITES];

template <class T>
__device__ __forceinline__ void sr_uniform_check(int site, int line, const T& x) {
    static_assert(sizeof(T) == 4, "an SGPR operand");
    const int b = __builtin_bit_cast(int, x);
    const bool bad = __ballot(b != __builtin_amdgcn_readfirstlane(b)) != 0;
    const int lane = (int)__lane_id();
    if (lane == __builtin_amdgcn_readfirstlane(lane)) {  // the first active lane
        atomicAdd(&sr_u_count[0][site], 1u);
        if (bad) atomicAdd(&sr_u_count[1][site], 1u);
        sr_u_line[site] = line;
    }
}
#define SR_UCHK(site, x) sr_uniform_check(SR_U_##site, __LINE__, x)

#else
#define SR_UCHK(site, x) ((void)0)
#endif  // SR_CHECK_UNIFORM

#define SR_PIN(site, x)                \
    do {                               \
        SR_UCHK(site, x);              \
        asm volatile("" : "+s"(x));    \
    } while (0)
#define SR_PIN6(s0, a, s1, b, s2, c, s3, d, s4, e, s5, f)                                \
    do {                                                                                 \
        SR_UCHK(s0, a);                                                                  \
        SR_UCHK(s1, b);                                                                  \
        SR_UCHK(s2, c);                                                                  \
        SR_UCHK(s3, d);                                                                  \
        SR_UCHK(s4, e);                                                                  \
        SR_UCHK(s5, f);                                                                  \
        asm volatile("" : "+s"(a), "+s"(b), "+s"(c), "+s"(d), "+s"(e), "+s"(f));         \
    } while (0)
#define SR_KEEP(site, x)                       \
    do {                                       \
        SR_UCHK(site, x);                      \
        asm volatile("; keep %0" ::"s"(x));    \
    } while (0)
// the same use of a per-lane value: asserts nothing, no site
#define SR_KEEP_LANE(x) asm volatile("; keep %0" ::"v"(x))
#define SR_RFL(site, x) (SR_UCHK(site, x), __builtin_amdgcn_readfirstlane(x))

#ifdef SR_CHECK_UNIFORM
// One 64-lane wave through the very macros above: the lane index (bad), a
// constant, a NaN constant (bits are compared, NaN != NaN is not), and a value
// equal among the lanes of a divergent branch and never evaluated by the
// others (the exec mask is honoured). `sink` keeps the operands alive.
__global__ __launch_bounds__(64) void sr_uniform_selftest_kernel(int* __restrict__ sink, float c, float nanv) {
    int lane = (int)threadIdx.x;
    int acc = SR_RFL(SELF_LANE, lane);
    SR_PIN(SELF_CONST, c);
    SR_PIN(SELF_NAN, nanv);
    acc += __builtin_bit_cast(int, c) ^ __builtin_bit_cast(int, nanv);
    int v = lane;  // what the even lanes' register may still hold inside the branch
    if (threadIdx.x & 1) {
        v = sink[64 + (threadIdx.x & 1)];  // one word, read by the odd lanes only
        acc += SR_RFL(SELF_BRANCH, v);
    }
    acc += v;
    sink[threadIdx.x] = acc;
}

// ---- host side: the checked build's entry points ---------------------------
extern "C" int sr_debug_uniform_sites(void) { return SR_U_NSITES; }
extern "C" int sr_debug_uniform_reset(void) {
    if (hipDeviceSynchronize() != hipSuccess) return -3;
    static const unsigned z[2][SR_U_NSITES] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(sr_u_count), z, sizeof z) == hipSuccess ? 0 : -3;
}
// seen[n], bad[n]: waves per site since the last reset, n = sr_debug_uniform_sites()
extern "C" int sr_debug_uniform_read(unsigned* seen, unsigned* bad, int n) {
    if (n != SR_U_NSITES) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -3;
    if (hipMemcpyFromSymbol(seen, HIP_SYMBOL(sr_u_count), n * sizeof(unsigned)) != hipSuccess) return -3;
    if (hipMemcpyFromSymbol(bad, HIP_SYMBOL(sr_u_count), n * sizeof(unsigned), n * sizeof(unsigned)) != hipSuccess)
        return -3;
    return 0;
}
// The site table: a site's name (static storage; nullptr past the end) and
// its line in geodesic.hip / uniform.h (0: no wave has reached it yet).
extern "C" const char* sr_debug_uniform_site_name(int site) {
    static const char* const names[] = {
#define SR_USITE_NAME(n) #n,
        SR_USITES(SR_USITE_NAME)
#undef SR_USITE_NAME
    };
    return site >= 0 && site < SR_U_NSITES ? names[site] : nullptr;
}
extern "C" int sr_debug_uniform_lines(int* lines, int n) {
    if (n != SR_U_NSITES) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -3;
    return hipMemcpyFromSymbol(lines, HIP_SYMBOL(sr_u_line), n * sizeof(int)) == hipSuccess ? 0 : -3;
}
// Launches the self-test's wave (it counts at the four SELF_* sites).
extern "C" int sr_debug_uniform_selftest(void) {
    int* sink = nullptr;
    if (hipMalloc(&sink, 128 * sizeof(int)) != hipSuccess) return -3;
    int rc = hipMemset(sink, 0, 128 * sizeof(int)) == hipSuccess ? 0 : -3;
    if (!rc) {
        hipLaunchKernelGGL(sr_uniform_selftest_kernel, dim3(1), dim3(64), 0, 0, sink, 1.5f, __builtin_nanf(""));
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = -3;
    }
    (void)hipFree(sink);
    return rc;
}
#endif  // SR_CHECK_UNIFORM

#endif  // SR_UNIFORM_H
