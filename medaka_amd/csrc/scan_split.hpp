// Splitting the scan: the latency-bound batches of the reference (100-200 windows of 10 000 columns) become the
// throughput-bound batch the chip is good at.
//
// A window is T dependent steps per layer and direction, and a batch of 200 windows has work for 100 of the 256 CUs
// (rec_mfma.hpp: one work-group per 4 windows and direction).  But a GRU forgets: started from h = 0 a few hundred
// columns before column a, both layers arrive at column a in the state the full scan has there, to within rounding
// (measured on the engine: profiles/r3_experiments/scan_split/merge_probe.txt) -- the property the reference itself
// relies on when it cuts contigs into 10 000-column windows that overlap by 1000 and stitches them at the middle of
// the overlap (medaka/medaka.py:266-272, medaka/stitch.py:169-194).  So every window is cut into S chunks, each
// extended by a margin of G columns on both sides, and the S*B "virtual windows" go through the unchanged kernels
// as ONE batch of T/S + 2G columns.
//
// Nothing is taken on trust: every junction is CERTIFIED on the device before the call returns.  For both layers and
// both directions, the state the warm-started chunk has at the junction (and again G/2 columns further along its scan)
// is compared with the state its neighbour carried there through its whole chunk; if any of these differ by more
// than kSplitEps (2^-18; 2^-10 in half-precision mode) the call is repeated with the next larger margin (which later calls then
// start from), and once the margin would pass kSplitMarginMax, as the plain sequential scan -- and the model stays
// sequential from then on.
//
//   virtual window v = k*B + w  = columns [start[k], start[k] + Tv) of window w; its columns [core0[k], core0[k+1])
//   are the ones that are delivered (SplitPlan, layout.hpp): the classifier head writes exactly those, straight into
//   the (B, T, 5) result (head.hpp).
#pragma once
#include "common.hpp"
#include "layout.hpp"

namespace mdk {

constexpr int kSplitMarginMax = 512;      // auto mode climbs a ladder of margins up to here (split_policy.hpp kMarginLadder), then gives the model up
constexpr int kSplitFlagWords = 8 * (kMaxSplit - 1);   // certificate words on the device: one per certificate point
// Largest junction difference that certifies, on h in [-1, 1].  Two scans that have merged still differ by the rounding
// noise of their different histories, and how large that is depends on the MODEL (its gains amplify the 2^-22 of the fp16
// hi/lo operands): 4e-7 .. 8e-7 for five of the seven trained weight sets of round 4, 1.1e-6 .. 2.4e-6 for the
// run-length-correction set `hp` (profiles/r4_split_evidence.json, r4_split_margins.json); half-precision mode (11 bits)
// 1e-5 .. 2e-4.  Scans that have NOT merged show 8.5e-6 (margin 96 of the round-1 set), 1.2e-5 (`hp` at 128), 2e-4 and up.
// Round 3's 2^-19 sat INSIDE `hp`'s noise band: that model was rejected on most inputs although a wider margin changed
// nothing (2.3e-6 at 512 as at 192).  Round 4 moved to 2^-17 = 7.6e-6, only 10 % under the smallest UNMERGED difference on
// record (8.5e-6): too close for models outside the seven-set zoo.  2^-18 = 3.8e-6 keeps 1.6 x above `hp`'s noise band and
// 2.2 x below that unmerged case (the one merged pair above it, `depthmix` at a margin of 64 with 5.4e-6, simply keeps its
// margin of 96); the probabilities then differ by about half the state difference (measured), an order of magnitude
// inside the audit tolerance below -- which is independent of this threshold -- and two inside the contract's 1e-4.
// Half precision: 2^-10 (2 ulp of the fp16 image it keeps of h).
constexpr float kSplitEps = 3.814697265625e-06f;      // 2^-18
constexpr float kSplitEpsHalf = 9.765625e-04f;        // 2^-10
// Audit threshold on the probabilities (split result vs the sequential scan of the same call): measured 2.4e-7 .. 1.2e-6
// (fp32 parity) and 1e-6 (half) on certified calls; the contract tolerance is 1e-4.
constexpr float kAuditTol = 1.0e-5f;
constexpr float kAuditTolHalf = 4.0e-4f;

// x (B, T, F) -> xv (S*B, Tv, F), local columns [t_lo, t_lo + nt) of every virtual window: rows of nt*F floats, copied as
// float2 (every row starts on a multiple of 2*F floats only when F is even: the odd case falls back to scalar copies
// through `vec` = 1).  The whole batch is t_lo = 0, nt = Tv.  `cond`: run only if *cond != 0 -- the fused layer 0 packs its
// operands straight from x (k_pack_x); the virtual batch is materialised only for the exact-projection fallback that an input
// beyond fp16 range switches to on the device (k_pack_x raises the flag).
static __global__ __launch_bounds__(256) void k_split_gather(const float *__restrict__ x, float *__restrict__ xv,
                                                             SplitPlanCore p, int F, int vec, int t_lo, int nt, const int *__restrict__ cond,
                                                             const int *__restrict__ gate) {
    if (gated_off(gate)) return;          // predicated pass (common.hpp)
    if (cond != nullptr && *cond == 0) return;
    const long row_elems = (long)nt * F / vec;
    const long total = (long)p.S * p.B * row_elems;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long v = i / row_elems, e = i - v * row_elems;
        const int k = (int)(v / p.B), w = (int)(v - (long)k * p.B);
        const size_t src = ((size_t)w * p.T + p.start[k] + t_lo) * F;
        const size_t dst = ((size_t)v * p.Tv + t_lo) * F;
        if (vec == 2)
            reinterpret_cast<float2 *>(xv + dst)[e] = reinterpret_cast<const float2 *>(x + src)[e];
        else
            xv[dst + e] = x[src + e];
    }
}

// h of (virtual window v, local column t, direction d, unit u) in an activation buffer (layout.hpp act_t)
__device__ __forceinline__ float split_h(const float *__restrict__ act, int Tv, int v, int t, int d, int u) {
    const int tile = v >> 3, wt = v & 7;
    const int lane = (wt >> 1) * 16 + (u & 15);
    return act[act_block(2, tile, Tv, t) + act_in_block(d, u >> 4, wt & 1, lane)];
}

// Certificate.  Block (x, y): 8 windows of certificate point y = ((j * 2 + layer) * 2 + direction) * 2 + point, one
// thread per hidden unit; flag[y] = bits of the largest |h_carried - h_warm| of that point (the host compares them
// with the threshold: non-negative floats order like their bit patterns; not-a-number counts as infinite).
//   direction 0 scans t upwards: at real column a = core0[j+1], chunk j carried its state to a - 1 (and on into its
//   right margin); chunk j+1 arrives there warm.  Direction 1 scans downwards: chunk j+1 carried its state to a (and on
//   into its left margin), chunk j arrives there warm.  Point 1 is G/2 columns further along the scan: both chunks have
//   run on from the junction, and the differences must still be below eps there (not further out: in the outer half of
//   a margin layer 1 is fed by a layer 0 that is itself still warming up in the other direction, by design).
constexpr int kVerifyWin = 8;
static __global__ __launch_bounds__(128) void k_split_verify(const float *__restrict__ act0, const float *__restrict__ act1,
                                                             SplitPlanCore p, unsigned *__restrict__ flag) {
    const int u = threadIdx.x;
    int z = blockIdx.y;
    const int point = z & 1; z >>= 1;
    const int d = z & 1; z >>= 1;
    const int layer = z & 1; z >>= 1;
    const int j = z;
    const float *act = layer ? act1 : act0;
    const int a = p.core0[j + 1];
    const int t = d == 0 ? (a - 1 + point * (p.G / 2)) : (a - point * (p.G / 2));
    float worst = 0.f;
    for (int w = blockIdx.x * kVerifyWin; w < min(p.B, (int)(blockIdx.x + 1) * kVerifyWin); ++w) {
        const float h0 = split_h(act, p.Tv, j * p.B + w, t - p.start[j], d, u);
        const float h1 = split_h(act, p.Tv, (j + 1) * p.B + w, t - p.start[j + 1], d, u);
        float delta = fabsf(h0 - h1);
        if (!(delta <= 4.0f)) delta = __builtin_inff();      // not a number
        worst = fmaxf(worst, delta);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) worst = fmaxf(worst, __shfl_xor(worst, o));
    if ((threadIdx.x & 63) == 0 && worst > 0.f) atomicMax(&flag[blockIdx.y], __float_as_uint(worst));
}

// Audit (first certified call of a model, and again whenever its margin has changed): the largest |a - b| over two
// probability arrays -- the split result against the sequential scan of the same call.  flag[0] = its bit pattern.
static __global__ __launch_bounds__(256) void k_split_audit(const float *__restrict__ a, const float *__restrict__ b, size_t n,
                                                            unsigned *__restrict__ flag, const int *__restrict__ gate = nullptr) {
    if (gated_off(gate)) return;          // predicated audit of the stream-ordered entry: only behind a certified split
    float worst = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float d = fabsf(a[i] - b[i]);
        if (!(d <= 4.0f)) d = __builtin_inff();
        worst = fmaxf(worst, d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) worst = fmaxf(worst, __shfl_xor(worst, o));
    if ((threadIdx.x & 63) == 0 && worst > 0.f) atomicMax(&flag[0], __float_as_uint(worst));
}

// ---- the stream-ordered entry (mdk_gru_forward_dev_async, gru_split.hpp): the decision on the device
// One set of these words per model.  The gates predicate the passes behind the split (common.hpp gated_off); the record is what
// the host's bookkeeping is later fed from (copied to a page-locked ring slot at the end of the call).
struct AsyncRecord {
    float worst;            // largest junction difference of the split (certificate words of k_split_verify)
    int certified;          // 1: the split is delivered -- its certificate held, and the probe it was gated on (if any)
    float probe_delta;      // half precision: largest junction difference of the fp32-parity probe the call was gated on
    int probe_ok;           // ... and that probe's verdict (1 when no probe gated the call)
    unsigned audit_bits;    // k_split_audit: largest |p_split - p_sequential| (0: not audited, or the split was rejected)
    int pad[3];
};
struct AsyncWords {
    float probe_delta;      // the last probe's verdict, kept across calls: a later call at its margin is gated on it
    int probe_ok;
    int gate[2];            // [0] the repair (sequential passes): 1 = skip, the split is certified; [1] the audit: 1 = skip
    AsyncRecord rec;        // this call's record -- it and the gates are zeroed at the start of every call
};

// One wave: reduce the certificate words (and the words of this call's probe, `probe` = 1, or the kept verdict of an earlier
// call's probe at the same margin, `probe` = 2) against the thresholds, write the gates and the record.  Non-negative floats order
// like their bit patterns; not-a-number was stored as infinity by k_split_verify.
static __global__ __launch_bounds__(64) void k_split_decide(const unsigned *__restrict__ flag, const unsigned *__restrict__ probe_flag,
                                                             int n, float eps, int probe, AsyncWords *__restrict__ w) {
    const int lane = threadIdx.x;
    float worst = 0.f, pworst = 0.f;
    for (int i = lane; i < n; i += 64) {
        worst = fmaxf(worst, __uint_as_float(flag[i]));
        if (probe == 1) pworst = fmaxf(pworst, __uint_as_float(probe_flag[i]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        worst = fmaxf(worst, __shfl_xor(worst, o));
        pworst = fmaxf(pworst, __shfl_xor(pworst, o));
    }
    if (lane != 0) return;
    if (probe == 1) { w->probe_delta = pworst; w->probe_ok = pworst <= kSplitEps ? 1 : 0; }
    const bool pok = probe == 0 || w->probe_ok != 0;
    const bool ok = worst <= eps && pok;
    w->gate[0] = ok ? 1 : 0;
    w->gate[1] = ok ? 0 : 1;
    w->rec.worst = worst;
    w->rec.certified = ok ? 1 : 0;
    w->rec.probe_delta = probe ? w->probe_delta : 0.f;
    w->rec.probe_ok = pok ? 1 : 0;
}

// A failed audit of the stream-ordered entry: the sequential result replaces the split's in `probs` -- a copy that runs only
// behind a certified split (`gate`) whose audit found more than `tol` (a hipMemcpyAsync cannot be predicated)
static __global__ __launch_bounds__(256) void k_audit_deliver(float *__restrict__ probs, const float *__restrict__ audit, size_t n,
                                                              const int *__restrict__ gate, const unsigned *__restrict__ dp_bits, float tol) {
    if (gated_off(gate)) return;
    if (__uint_as_float(__builtin_amdgcn_readfirstlane(*dp_bits)) <= tol) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) probs[i] = audit[i];
}

}  // namespace mdk
