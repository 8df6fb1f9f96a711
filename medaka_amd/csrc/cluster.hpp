// The cluster recurrence shared by the read-level LSTM(384) (k_lstm_wide, lstm_wide.hpp) and the GRU(256) (k_gru_wide,
// gru_wide.hpp): placement handshake, h exchange, register-resident W_hh contraction and step schedule; and on the host its
// launch plan, time-out word, retry policy and W_hh fragment order.  A kernel supplies only its cell (gate math, gi slot,
// carried state, per-unit setup) and its addressing.
//
// One direction's recurrent matrix (4H or 3H rows x H as fp16 hi/lo fragments) does not fit the registers + LDS of one CU,
// and re-streaming it from L2 every step would cost microseconds per step.  So the H hidden units are split over a CLUSTER
// of H / 32 work-groups (= CUs):
//
//   * member m owns units [32m, 32m+32); its wave w8 owns the 16 W rows (gate n & 3 of unit 32m + 4*w8 + n / 4) with their
//     fragments resident in registers (H / 32 k-steps x hi/lo).  W is the *A* operand of the MFMA and h the B operand
//     (columns = windows), so the accumulator of lane (g, c) holds the gates of unit g for window c: the cell update needs
//     no cross-lane traffic (fp32-parity mode: one DPP add joins the hi and lo columns of a window);
//   * every step each member needs the WHOLE h_{t-1} (8 rows x H units).  Members publish their 32 units as 8-byte
//     {fp16 hi, fp16 lo, step tag} granules, one 8-byte store each, and gather all granules of the step with 16-byte
//     L1-bypassing (sc1) loads, re-polling until each 8-byte half carries the current tag: the data-tagged granule needs no
//     flag and no fence (MI355X_MICROARCH.md, hand-off form R2).  The stores are agent-scope atomics (write-through, valid
//     across XCDs) unless the members verified at kernel start that they share one XCD, in which case plain stores that
//     stay in that XCD's L2 are several times faster.  Two parity buffers suffice: nobody can publish step t+2 before
//     everybody has gathered step t;
//   * the gathered granules are written into the LDS A-operand image layout of the 128-unit kernel (rec_mfma.hpp), H / 32
//     k-steps long; rows = (window, hi|lo) as there;
//   * above as many groups as clusters, two 8-window groups are interleaved per cluster so that one group's exchange latency
//     is covered by the other group's MFMAs;
//   * HP: half precision (`TorchModel.half()`): fp16 operands without the hi/lo split -- one A row per window, so a group is
//     16 windows (4 per lane) and W_hi only; a granule carries the fp16 h of TWO windows (2wp, 2wp+1), which makes the
//     exchange byte-for-byte the same code as the (hi, lo) granules of the fp32-parity mode.
//
// Cluster members must be co-resident (they spin on each other): one 512-thread work-group per CU, on an otherwise idle
// device; work-group b lands on XCD b % 8 (observed, used for speed only: a cluster shares one L2), and every spin is
// bounded -- on time-out the kernel raises `status[0]` and exits instead of hanging.
#pragma once
#include <chrono>
#include <thread>

#include "common.hpp"
#include "host_common.hpp"
#include "rec_mfma.hpp"

namespace mdk {

constexpr int kWWin = 8;                       // windows per group (fp32-parity rows = 16)
constexpr int kWMaxClusters = 16;              // per exchange buffer (= per direction): 2 per XCD
constexpr int kWidePF = 3;                     // gi prefetch ring depth of both kernels
constexpr int kWSpinLimit = 1 << 20;           // ~1-2 s of polling before giving up (a member died mid-kernel: never seen)
// The placement handshake is where a cluster finds out that its members are NOT all resident (not enough CUs free: another
// tenant holds them).  It is bounded in wall-clock time, not in polls: 50 ms of the constant 100 MHz clock (s_memrealtime)
// -- launch skew between resident work-groups is microseconds, a foreign kernel may hold CUs for a few milliseconds -- so
// that a GPU that cannot host the kernel is reported within ~0.1 s instead of after seconds of spinning.
constexpr unsigned long long kWHandshakeTicks = 5000000ull;

// One exchange buffer for hidden width H: per cluster [2 groups][2 parities][8 rows][H] granules, then 16 header words (one
// 128-byte line) per cluster for the placement handshake.  Zeroed before every launch: tags restart at 1.
constexpr size_t wide_exch_words(int H) {
    return (size_t)kWMaxClusters * 4 * kWWin * H + (size_t)kWMaxClusters * 16;
}

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

__device__ __forceinline__ void raise_status(int *status) {
    if (threadIdx.x == 0) atomicExch(status, 1);
}

// blockIdx.x -> cluster and member: consecutive work-groups go to consecutive XCDs, so the members of a cluster are
// 8 apart (8 XCDs x 2 clusters x H / 32 members per launch row).
struct ClusterSlot { int cluster, member; };
template <int H>
__device__ __forceinline__ ClusterSlot cluster_slot() {
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    return {(idx / (H / 32)) * 8 + xcd, idx % (H / 32)};
}
// this lane's hidden unit: member m, wave w8, accumulator rows of lane group g
__device__ __forceinline__ int cluster_unit(int member) {
    const int tid = threadIdx.x;
    return 32 * member + 4 * __builtin_amdgcn_readfirstlane(tid >> 6) + ((tid & 63) >> 4);
}

// Placement handshake: do all members share an XCD (= one L2)?  Then plain stores (kept in that L2) + L1-bypassing loads
// are coherent and several times faster than write-through granules that every reader must fetch from the fabric.
// Placement is only OBSERVED to be block % 8, so the members tell each other their XCC_ID through the always-valid
// write-through protocol first and all take the same decision from the same values.
// Returns -1: a member did not show up within kWHandshakeTicks (the caller raises the status and exits),
// 0: write-through granules, 1: same XCD.
template <int H>
__device__ __forceinline__ int cluster_handshake(unsigned long long *exch, int cluster, int member) {
    constexpr int NC = H / 32;
    static_assert(NC <= 16, "one 16-word header per cluster");
    __shared__ int s_same;
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned long long *hdr = exch + (size_t)kWMaxClusters * (4 * kWWin * H) + (size_t)cluster * 16;
    const unsigned int xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xf;   // HW_REG_XCC_ID[3:0]
    if (tid == 0)
        __hip_atomic_store(hdr + member, (0x7fffffffull << 32) | xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < 64) {
        unsigned long long x = 0;
        const unsigned long long t_begin = __builtin_amdgcn_s_memrealtime();
        bool ok;
        do {
            if (lane < NC) x = __hip_atomic_load(hdr + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok = lane >= NC || (unsigned int)(x >> 32) == 0x7fffffffu;
            if (!__all(ok)) __builtin_amdgcn_s_sleep(4);
        } while (!__all(ok) && __builtin_amdgcn_s_memrealtime() - t_begin < kWHandshakeTicks);
        const bool same = lane >= NC || ((unsigned int)x & 0xf) == xcc;
        if (lane == 0) s_same = (__all(ok) && __all(same)) ? 1 : (__all(ok) ? 0 : -1);
    }
    __syncthreads();
    return s_same;
}

// This member's W_hh fragments, [H / 32 k-steps][hi, lo] per lane (half precision: hi only).  A kernel loads them before the
// placement handshake, so that their latency hides under it.
template <int H, bool HP>
struct WideW { half8 f[H / 32][HP ? 1 : 2]; };
template <int H, bool HP>
__device__ __forceinline__ WideW<H, HP> load_wide_w(const half8 *__restrict__ wfrag, int member) {
    constexpr int KS = H / 32;
    WideW<H, HP> w;
    const half8 *wp = wfrag + ((size_t)(member * 8 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6)) * (KS * 2)) * 64 +
                      (threadIdx.x & 63);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int sp = 0; sp < (HP ? 1 : 2); ++sp) w.f[ks][sp] = wp[(size_t)(ks * 2 + sp) * 64];
    return w;
}

template <int BYTES>
__device__ __forceinline__ void zero_image(unsigned char *im) {
    uint32_t *z = reinterpret_cast<uint32_t *>(im);
    for (int i = threadIdx.x; i < BYTES / 4; i += 512) z[i] = 0u;
}

// The scan of one cluster member over its units of work (NGRP consecutive groups each), steps [s0, s_end) of every window.
// Cell supplies:
//   H, GI (gi values per unit, the gi row is GI * H wide, this lane's at GI * unit), NG (gates of the contraction used),
//   gi_t + load_gi(p): one gi slot;
//   state0(live, win): the carried state of window win at s0 (live: the group exists, x < NGRP);
//   image0(img, live, win0, t_prev, g_off): the A image the first step reads (h of scan column t_prev, or h_0 = 0);
//   step(pre, gi, state, live) -> h: the cell (live: step < s_end);
//   save(win, state): after the unit.
// w: load_wide_w; gi / out point at this direction's column 0 (out rows are ldo wide); exch is this direction's exchange buffer.
template <int PF, int NGRP, bool HP, class Cell>
__device__ __forceinline__ void cluster_scan(const Cell &cell, WideW<Cell::H, HP> w, unsigned long long *exch,
                                             int *status, bool same_xcd, ClusterSlot cs, int n_clusters, int n_units,
                                             const float *__restrict__ gi, float *__restrict__ out, int ldo, int B, int T,
                                             int reverse, int s0, int s_end, int poll_delay)
{
    constexpr int H = Cell::H;
    constexpr int KS = H / 32;                     // k-steps of the contraction = members of a cluster
    constexpr int NJ = kWWin * H / 2 / 512;        // granule pairs per thread and step
    constexpr int GRAN = kWWin * H;                // granules per parity buffer
    constexpr int IMG = KS * kHKStride;            // bytes per A image
    constexpr int NS = HP ? 1 : 2;                 // fp16 pieces per operand
    constexpr int GW = HP ? 16 : 8;                // windows per group: column c = window (HP) or 2*window + {hi, lo}
    typedef typename Cell::gi_t gi_t;
    __shared__ __attribute__((aligned(16))) unsigned char img[2][2][IMG];   // [group][parity]
    __shared__ int s_abort[2];

    const int tid = threadIdx.x, lane = tid & 63;
    const int c = lane & 15, g = lane >> 4;     // accumulator: rows 4g..4g+3 = gates of unit g, column c
    const int wl = HP ? c : (c >> 1);           // this lane's window within the group
    const bool lead = HP || !(c & 1);           // fp32-parity: the hi column's lane finishes the cell

    half8 (&wf)[KS][NS] = w.f;
    const int unit = cluster_unit(cs.member);
    unsigned long long *ex = exch + (size_t)cs.cluster * (4 * GRAN);
    if (tid < 2) s_abort[tid] = 0;

    // gather: 4 H granule PAIRS (units u, u+1 of one row) per step; thread t takes pairs t + 512 j with one 16-byte sc1 load
    // each -- every load instruction of a wave covers 1 KB of contiguous memory -- and writes the fp16 hi pair / lo pair
    // with two 4-byte LDS stores.  (Each 8-byte half carries its own tag, so a torn 16-byte load is harmless.)
    int g_off[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int gidx = 2 * (tid + 512 * j);
        const int w = gidx / H, u = gidx % H;
        g_off[j] = (u >> 5) * kHKStride + ((u >> 3) & 3) * kHGroupStride + (2 * w) * 16 + (u & 7) * 2;
    }
    const int rd_off = g * kHGroupStride + c * 16;
    const long tstep = reverse ? -1 : 1;
    const int t_first = reverse ? (T - 1 - s0) : s0;
    const long gstride = tstep * (long)(Cell::GI * H), ostride = tstep * (long)ldo;

#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int sp = 0; sp < NS; ++sp) asm volatile("" ::"v"(wf[ks][sp]));

    unsigned int tag = 0;
    for (int it = cs.cluster; it < n_units; it += n_clusters) {   // unit of work = NGRP consecutive groups
        const float *gp[2];
        float *op[2];
        bool wok[2];
        float st[2];
        gi_t gq[2][PF];
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            int win = (NGRP * it + x) * GW + wl;
            wok[x] = win < B;
            if (!wok[x]) win = B - 1;
            gp[x] = gi + ((size_t)win * T + t_first) * (Cell::GI * H) + Cell::GI * unit;
            op[x] = out + ((size_t)win * T + t_first) * ldo + unit;
            st[x] = cell.state0(x < NGRP, win);
        }
        __syncthreads();                                  // previous unit's images are dead
#pragma unroll
        for (int x = 0; x < 2; ++x) cell.image0(img[x][tag & 1], x < NGRP, (NGRP * it + x) * GW, (long)t_first - tstep, g_off);
        auto refill = [&](int x, int p, bool advance) {
            gq[x][p] = cell.load_gi(gp[x]);
            if (advance) gp[x] += gstride;
        };
#pragma unroll
        for (int x = 0; x < 2; ++x) {
#pragma unroll
            for (int p = 0; p < PF; ++p) gq[x][p] = gi_t{};
#pragma unroll
            for (int p = 0; p + 1 < PF; ++p) refill(x, p, s0 + p + 1 < s_end);
        }
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int p = 0; p + 1 < PF; ++p)
#pragma unroll
                for (int e = 0; e < Cell::GI; ++e) asm volatile("" ::"v"(gq[x][p][e]));
        __syncthreads();

        // One half-step: compute + publish step `tag` of group x, and gather step `gtag` of the OTHER group (published one
        // half-step ago) into its next image:
        //     [C_A(t) + G_B(t-1)]  barrier  [C_B(t) + G_A(t)]  barrier     (C = compute + publish, G = gather)
        // NGRP = 1: one group per cluster, the exchange latency is exposed every step -- used while the batch has no more
        // groups than clusters (then more clusters run in parallel instead).  Vector-memory issue order is
        // [gather loads] [gi refill] ... [publish + h stores] [wait gather]: the wait covers only the gather loads (vmcnt
        // retires in order) whose data arrived under the MFMAs; the refill and the stores drain during the next half-step.
        // The barrier is LDS-only for the same reason.
        auto gather_issue = [&](int y, unsigned int gtag, uint4 (&v)[NJ]) {
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(ex + (size_t)(2 * y + (gtag & 1)) * GRAN, 0, GRAN * 8, 0x00020000);
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                v[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (tid + 512 * j) * 16, 0, 16));
        };
        auto gather_finish = [&](int y, unsigned int gtag, uint4 (&v)[NJ]) {
            unsigned char *wb = img[y][gtag & 1];
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(ex + (size_t)(2 * y + (gtag & 1)) * GRAN, 0, GRAN * 8, 0x00020000);
            int spins = 0;
            bool bad;
            do {
                bad = false;
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    if (v[j].y != gtag || v[j].w != gtag) {
                        bad = true;
                        v[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (tid + 512 * j) * 16, 0, 16));
                    }
                if (bad) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > kWSpinLimit) { s_abort[tag & 1] = 1; break; }
                }
            } while (bad);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                *reinterpret_cast<unsigned int *>(wb + g_off[j]) = (v[j].x & 0xffffu) | (v[j].z << 16);
                *reinterpret_cast<unsigned int *>(wb + g_off[j] + 16) = (v[j].x >> 16) | (v[j].z & 0xffff0000u);
            }
        };
        auto half_step = [&](int x, int p, int step, bool do_gather, unsigned int gtag) {
            const unsigned char *rb = img[x][(tag - 1) & 1];
            // the other group published early in the previous half-step: its granules are in L2 by now
            uint4 v[NJ];
            if constexpr (NGRP == 2) { if (do_gather) gather_issue(1 - x, gtag, v); }
            // gi prefetch is issued AFTER the gather loads: vmcnt retires in order, so this half-step's
            // gather wait does not include it and it has until the next half-step's to arrive
            if constexpr (NGRP == 2) refill(x, (p + PF - 1) % PF, (step + PF) < s_end);    // the slot consumed one step ago
            __builtin_amdgcn_sched_barrier(0);
            floatx4 acc0 = floatx4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#pragma unroll
            for (int ks = 0; ks < KS; ks += 2) {
                const half8 a0 = *reinterpret_cast<const half8 *>(rb + ks * kHKStride + rd_off);
                const half8 a1 = *reinterpret_cast<const half8 *>(rb + (ks + 1) * kHKStride + rd_off);
                acc0 = mfma16(wf[ks][0], a0, acc0);          // A = W (rows = gate rows), B = h (columns = windows)
                acc1 = mfma16(wf[ks + 1][0], a1, acc1);
                if constexpr (!HP) {
                    acc0 = mfma16(wf[ks][1], a0, acc0);
                    acc1 = mfma16(wf[ks + 1][1], a1, acc1);
                }
            }
            // acc[r] = gate r of unit g for column c; fp32-parity: add the lo column (lane c ^ 1)
            float pre[Cell::NG];
#pragma unroll
            for (int r = 0; r < Cell::NG; ++r) {
                float dot = acc0[r] + acc1[r];
                if constexpr (!HP) dot += dpp_mov<0xB1>(dot);     // quad_perm:[1,0,3,2]
                pre[r] = dot;
            }
            const float h = cell.step(pre, gq[x][p], st[x], step < s_end);
            unsigned int payload;
            if constexpr (HP) {   // a granule carries windows (2wp, 2wp + 1): take the odd neighbour's half
                const unsigned int hb = __builtin_bit_cast(unsigned short, (_Float16)(h * kActScale));
                const unsigned int nb = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)hb, 0xB1, 0xf, 0xf, true);
                payload = hb | (nb << 16);
            } else {
                _Float16 hi, lo;
                split_f16(h * kActScale, hi, lo);
                payload = (unsigned int)__builtin_bit_cast(unsigned short, hi) |
                          ((unsigned int)__builtin_bit_cast(unsigned short, lo) << 16);
            }
            unsigned long long *dst = ex + (size_t)(2 * x + (tag & 1)) * GRAN;
            if (!(c & 1)) {       // granule row c >> 1: (window, hi|lo) or a pair of windows
                const unsigned long long gran = ((unsigned long long)tag << 32) | payload;
                if (same_xcd)
                    __hip_atomic_store(dst + (c >> 1) * H + unit, gran, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);   // plain store: stays in the shared L2
                else
                    __hip_atomic_store(dst + (c >> 1) * H + unit, gran, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);       // write-through (sc1)
            }
            if (lead && step < s_end && wok[x]) op[x][0] = h;
            op[x] += ostride;
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (NGRP == 1) {
                // own group, just published: a poll that misses costs a second L2 round trip, so give the
                // other members' stores time to land first
                for (int i = 0; i < poll_delay; ++i) __builtin_amdgcn_s_sleep(1);
                gather_issue(x, gtag, v);
            }
            if (do_gather) gather_finish(NGRP == 2 ? 1 - x : x, gtag, v);
            if constexpr (NGRP == 1) refill(x, (p + PF - 1) % PF, (step + PF) < s_end);
            lds_barrier();
        };

        for (int step0 = s0; step0 < s_end; step0 += PF) {
#pragma unroll
            for (int p = 0; p < PF; ++p) {
                const int step = step0 + p;      // steps >= s_end run too (stores masked): all members agree
                ++tag;
                if constexpr (NGRP == 2) {
                    half_step(0, p, step, step > s0, tag - 1);
                    half_step(1, p, step, true, tag);
                } else {
                    half_step(0, p, step, true, tag);
                }
                if (s_abort[tag & 1]) return raise_status(status);
            }
        }
        if constexpr (NGRP == 2) {   // B's last step: keeps "nobody publishes t+2 before everybody gathered t" across units
            uint4 v[NJ];
            gather_issue(1, tag, v);
            gather_finish(1, tag, v);
        }
        __syncthreads();
        if (s_abort[0] | s_abort[1]) return raise_status(status);
#pragma unroll
        for (int x = 0; x < NGRP; ++x)
            if (lead && wok[x]) cell.save((NGRP * it + x) * GW + wl, st[x]);
    }
}

// ---- host side

// Windows -> groups (kWWin windows, 2 kWWin in half precision) -> units of work (ngrp groups) -> clusters (at most cap).
// ngrp: two groups interleaved per cluster when there are more groups than clusters, unless ngrp_force (1 or 2) says.
// work_groups: those that must be co-resident; grid: whole launch rows of 8 XCDs (the kernels return past n_clusters).
struct WidePlan { int gw = 8, n_groups = 0, ngrp = 1, n_units = 0, n_clusters = 0, work_groups = 0, grid = 0; };
inline WidePlan plan_wide(int nb, bool hp, int cluster_size, int cap, int ngrp_force = 0) {
    WidePlan w;
    w.gw = hp ? 2 * kWWin : kWWin;
    w.n_groups = (nb + w.gw - 1) / w.gw;
    w.ngrp = w.n_groups > cap ? 2 : 1;
    if (ngrp_force == 1 || ngrp_force == 2) w.ngrp = ngrp_force;
    w.n_units = (w.n_groups + w.ngrp - 1) / w.ngrp;
    w.n_clusters = std::min(w.n_units, cap);
    w.work_groups = w.n_clusters * cluster_size;
    w.grid = 8 * cluster_size * ((w.n_clusters + 7) / 8);
    return w;
}

// Read the time-out word after the work queued on s and clear it: *raised = a cluster timed out (the result is lost).
inline int take_wide_status(int *status, hipStream_t s, int *raised) {
    int st = 0;
    HIP_TRY(hipMemcpyAsync(&st, status, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *raised = st != 0;
    if (st != 0) HIP_TRY(hipMemsetAsync(status, 0, sizeof(int), s));
    return MDK_OK;
}

// A time-out is not an error yet: every try is bounded on the device (the 50 ms handshake; later launches of a lost forward
// return at once), so the host re-runs the forward -- attempt(&timed_out) -- with a growing pause, 20, 40, ... 320 ms, until
// it goes through or waiting once more would pass wait_ms since t0; then give_up(tries, spent_ms).  Never a hang, never a
// wrong result.  tries: those already made since t0 without a pause.
template <class Attempt, class GiveUp>
inline int retry_wide(Attempt attempt, GiveUp give_up, int wait_ms, std::chrono::steady_clock::time_point t0, int tries = 0) {
    for (int pause_ms = 0;;) {
        int timed_out = 0;
        tries++;
        const int rc = attempt(&timed_out);
        if (rc || !timed_out) return rc;
        const long spent = (long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
        pause_ms = pause_ms ? std::min(2 * pause_ms, 320) : 20;
        if (spent + pause_ms > wait_ms) return give_up(tries, spent);
        std::this_thread::sleep_for(std::chrono::milliseconds(pause_ms));
    }
}

// W (rows = gate * H + unit, K columns) as fp16 hi/lo fragments in the tile order of the cluster kernels,
// [H / 4 tiles][K / 32 k-steps][hi, lo][64 lanes]: tile nt = member * 8 + wave, row n of the tile = gate (n & 3) of unit
// 32 * member + 4 * wave + (n >> 2); gates >= n_gates are zero rows.  W_hh for the kernels' registers, and the B operand of
// k_gemm_rows (permuted gi columns nt * 16 + n).
inline void pack_wide_tiles(half8 *dst, const float *w, int H, int K, int n_gates, float scale) {
    const int KS = K / 32;
    for (int nt = 0; nt < H / 4; ++nt)
        for (int lane = 0; lane < 64; ++lane) {
            const int n = lane & 15, kg = lane >> 4, gate = n & 3;
            const int j = gate * H + 32 * (nt / 8) + 4 * (nt % 8) + (n >> 2);
            for (int ks = 0; ks < KS; ++ks) {
                half8 hi, lo;
                for (int i = 0; i < 8; ++i) {
                    _Float16 a = (_Float16)0.f, b = (_Float16)0.f;
                    if (gate < n_gates) split_host(w[(size_t)j * K + 32 * ks + 8 * kg + i] * scale, a, b);
                    hi[i] = a; lo[i] = b;
                }
                const size_t base = (((size_t)nt * KS + ks) * 2) * 64 + lane;
                dst[base] = hi; dst[base + 64] = lo;
            }
        }
}

}  // namespace mdk
