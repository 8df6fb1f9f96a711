// GRU(256): the consensus GRU at the width `medaka train` builds by default (reference medaka/models.py DEFAULT_MODEL_DICT:
// GRUModel(num_features=10, num_classes=5, gru_size=256)).
//
// One direction's recurrent matrix is 768 x 256 = 786 KB as fp16 hi/lo fragments: more than the registers + LDS of one CU.
// The design is that of the read-level LSTM(384) (lstm_wide.hpp), brought to the GRU cell:
//
//   * a CLUSTER of 8 work-groups (= 8 CUs) per window group; member m owns units [32m, 32m+32); its wave w8 owns the 16
//     gate rows (r, z, n, 0) x units 32m + 4*w8 + 0..3 with their W_hh fragments resident in registers (8 k-steps x hi/lo =
//     64 VGPRs; the fourth row of a unit is zero, so that the accumulator of lane (g, c) is exactly (r, z, n) of unit g for
//     column c and the cell needs no cross-lane traffic -- fp32-parity mode: one DPP add joins the hi and lo columns);
//   * every step each member gathers the WHOLE h_{t-1} (8 rows x 256 units of 8-byte {fp16 hi, fp16 lo, step tag} granules)
//     from the members' publishes, exactly as k_lstm_wide does: data-tagged granules, no flag, no fence; plain stores when the
//     members verified at kernel start that they share one XCD, agent-scope write-through otherwise; two parity buffers;
//   * two groups are interleaved per cluster when the batch has more groups than clusters;
//   * the grid is [8 XCDs x clusters / 8 x 8 members] x directions: both directions of a layer run in one launch, each
//     direction its own clusters and exchange buffers;
//   * every spin is bounded (the 50 ms placement handshake, kWSpinLimit polls): a time-out raises `status[0]` and the kernel
//     exits; the host re-runs the forward or reports MDK_ERR_DEVICE (gru_wide_run.hpp).
//
// n = tanh(gi_n + r * (W_hn h + b_hn)), h' = n + z (h - n): gi (input projection with b_ih, and b_hr / b_hz folded) arrives
// pre-scaled by S = kActScale * sw like the accumulator, b_hn is scaled here.  The reverse direction scans T-1 .. 0 and writes
// column t.
#pragma once
#include "common.hpp"
#include "rec_mfma.hpp"
#include "lstm_wide.hpp"

namespace mdk {

constexpr int kGH = 256;                        // hidden units
constexpr int kGG = 3 * kGH;                    // gi columns per direction (permuted: 3 * unit + gate)
constexpr int kGC = 8;                          // work-groups (CUs) per cluster
constexpr int kGKS = kGH / 32;                  // k-steps of the recurrent contraction
constexpr int kGImgBytes = kGKS * kHKStride;    // 8 KB per A image
constexpr int kGGranules = kWWin * kGH;         // per parity buffer (8 rows)
constexpr int kGMaxClusters = 16;               // per direction
constexpr size_t kGExchPerDir = (size_t)kGMaxClusters * 4 * kGGranules + (size_t)kGMaxClusters * 16;   // + XCD headers

// Clusters of one launch: at most kGClusterBudget x 8 CUs for all directions of a process (`gpu_share` processes divide them), so
// that every member of every cluster can be resident at once on a GPU whose CUs the process shares with nothing else.
constexpr int kGClusterBudget = 28;     // 224 of 256 CUs
struct WidePlan { int gw = 8, n_groups = 0, ngrp = 1, n_units = 0, n_clusters = 0, work_groups = 0; };
inline WidePlan plan_wide(int nb, int D, bool hp, int gpu_share) {
    WidePlan w;
    const int cap = std::max(1, std::min(kGMaxClusters, kGClusterBudget / (D * gpu_share)));
    w.gw = hp ? 2 * kWWin : kWWin;
    w.n_groups = (nb + w.gw - 1) / w.gw;
    w.ngrp = w.n_groups > cap ? 2 : 1;                     // more groups than clusters: two interleaved per cluster
    w.n_units = (w.n_groups + w.ngrp - 1) / w.ngrp;
    w.n_clusters = std::min(w.n_units, cap);
    w.work_groups = D * w.n_clusters * kGC;
    return w;
}

// Layer 0's projection (F <= 16 features) in plain fp32 FMAs, for both precisions: x arrives unscaled and in any range --
// raw counts included, which an fp16 split would overflow -- and 768 x 16 FMAs per column are nothing beside the 3 KB of gi
// per column and direction this writes.  Thread t owns the four gi columns 4t .. 4t + 3 of direction blockIdx.y with their
// weights in registers; a work-group walks 64-row blocks, x staged in LDS.
//   gi[d][row][j'] = bias[d][j'] + sum_k x[row][k] * w[d][k][j']   (k ascending; w, bias pre-scaled by S, permuted order)
constexpr int kG0Rows = 64;
__global__ __launch_bounds__(192) void k_gi_wide0(
    const float *__restrict__ x,       // [M][K]
    const float *__restrict__ w,       // [D][K][768]
    const float *__restrict__ bias,    // [D][768]
    float *__restrict__ gi,            // [D][M][768]
    long M, int K)
{
    __shared__ float xs[kG0Rows][16];
    const int d = blockIdx.y, j = 4 * threadIdx.x;
    float4 wv[16];
#pragma unroll
    for (int k = 0; k < 16; ++k)
        wv[k] = k < K ? *reinterpret_cast<const float4 *>(w + ((size_t)d * K + k) * kGG + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 bv = *reinterpret_cast<const float4 *>(bias + (size_t)d * kGG + j);
    float *gd = gi + (size_t)d * M * kGG + j;
    for (long r0 = (long)blockIdx.x * kG0Rows; r0 < M; r0 += (long)gridDim.x * kG0Rows) {
        __syncthreads();
        for (int i = threadIdx.x; i < kG0Rows * 16; i += 192) {
            const int r = i >> 4, k = i & 15;
            xs[r][k] = (r0 + r < M && k < K) ? x[(size_t)(r0 + r) * K + k] : 0.f;
        }
        __syncthreads();
        const int nr = M - r0 < kG0Rows ? (int)(M - r0) : kG0Rows;
        for (int r = 0; r < nr; ++r) {
            float4 acc = bv;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const float xv = xs[r][k];
                acc.x = __builtin_fmaf(xv, wv[k].x, acc.x);
                acc.y = __builtin_fmaf(xv, wv[k].y, acc.y);
                acc.z = __builtin_fmaf(xv, wv[k].z, acc.z);
                acc.w = __builtin_fmaf(xv, wv[k].w, acc.w);
            }
            *reinterpret_cast<float4 *>(gd + (size_t)(r0 + r) * kGG) = acc;
        }
    }
}

// HP: half precision -- fp16 operands without the hi/lo split, 16 windows per group (as k_lstm_wide).
template <int PF, int NGRP, bool HP = false>
__global__ __launch_bounds__(512, 1) void k_gru_wide(
    const float *__restrict__ gi,       // [D][B*T][768] permuted gate columns, biases folded, PRE-SCALED by S
    const half8 *__restrict__ wfrag,    // [D][8 members][8 waves][8 ks][2 hi/lo][64]
    const float *__restrict__ b_hn,     // [D][256] unscaled
    const float *__restrict__ inv_scale_d,   // [D] 1 / S
    float *__restrict__ out,            // [B*T][D*256]: direction d writes units d*256 ..
    unsigned long long *exch,           // [D][kGExchPerDir] granules + headers, zeroed before the launch
    int *status,                        // [0] != 0: a cluster timed out
    int B, int T, int D, int n_clusters, int n_units, int poll_delay, int skip_if_lost)
{
    __shared__ __attribute__((aligned(16))) unsigned char img[2][2][kGImgBytes];   // [group][parity]
    __shared__ int s_abort[2];
    __shared__ int s_same;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int dir = blockIdx.y, reverse = dir;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int cluster = (idx / kGC) * 8 + xcd, member = idx % kGC;
    if (cluster >= n_clusters) return;
    if (skip_if_lost && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    const int c = lane & 15, g = lane >> 4;
    constexpr int NS = HP ? 1 : 2;
    constexpr int GW = HP ? 16 : 8;
    const int wl = HP ? c : (c >> 1);
    const bool lead = HP || !(c & 1);

    half8 wf[kGKS][NS];
    {
        const half8 *wp = wfrag + ((size_t)((dir * kGC + member) * 8 + w8) * (kGKS * 2)) * 64 + lane;
#pragma unroll
        for (int ks = 0; ks < kGKS; ++ks)
#pragma unroll
            for (int sp = 0; sp < NS; ++sp) wf[ks][sp] = wp[(size_t)(ks * 2 + sp) * 64];
    }
    constexpr float L2E = 1.44269504088896340736f;
    const float inv_scale = inv_scale_d[dir];
    const float c_sig = -L2E * inv_scale, c_tanh = 2.0f * L2E * inv_scale;
    const int unit = 32 * member + 4 * w8 + g;
    const float bhn = b_hn[dir * kGH + unit] * (1.0f / inv_scale);
    const int ldo = D * kGH;
    unsigned long long *ex_dir = exch + (size_t)dir * kGExchPerDir;
    unsigned long long *ex = ex_dir + (size_t)cluster * (4 * kGGranules);
    const float *gid = gi + (size_t)dir * B * T * kGG;
    float *outd = out + dir * kGH;
    if (tid < 2) s_abort[tid] = 0;

    // placement handshake and same-XCD decision (k_lstm_wide)
    {
        unsigned long long *hdr = ex_dir + (size_t)kGMaxClusters * (4 * kGGranules) + (size_t)cluster * 16;
        const unsigned int xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xf;   // HW_REG_XCC_ID[3:0]
        if (tid == 0)
            __hip_atomic_store(hdr + member, (0x7fffffffull << 32) | xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid < 64) {
            unsigned long long x = 0;
            const unsigned long long t_begin = __builtin_amdgcn_s_memrealtime();
            bool ok;
            do {
                if (lane < kGC) x = __hip_atomic_load(hdr + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = lane >= kGC || (unsigned int)(x >> 32) == 0x7fffffffu;
                if (!__all(ok)) __builtin_amdgcn_s_sleep(4);
            } while (!__all(ok) && __builtin_amdgcn_s_memrealtime() - t_begin < kWHandshakeTicks);
            const bool same = lane >= kGC || ((unsigned int)x & 0xf) == xcc;
            if (lane == 0) s_same = (__all(ok) && __all(same)) ? 1 : (__all(ok) ? 0 : -1);
        }
        __syncthreads();
        if (s_same < 0) {
            if (tid == 0) atomicExch(status, 1);
            return;
        }
    }
    const bool same_xcd = s_same == 1;

    // gather: 1024 granule PAIRS per step, thread t takes pairs t and t + 512 (one 16-byte sc1 load each)
    int g_off[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int gidx = 2 * (tid + 512 * j);
        const int w = gidx / kGH, u = gidx % kGH;
        g_off[j] = (u >> 5) * kHKStride + ((u >> 3) & 3) * kHGroupStride + (2 * w) * 16 + (u & 7) * 2;
    }
    const int rd_off = g * kHGroupStride + c * 16;
    const long tstep = reverse ? -1 : 1;
    const int t_first = reverse ? (T - 1) : 0;
    const long gstride = tstep * (long)kGG, ostride = tstep * (long)ldo;

#pragma unroll
    for (int ks = 0; ks < kGKS; ++ks)
#pragma unroll
        for (int sp = 0; sp < NS; ++sp) asm volatile("" ::"v"(wf[ks][sp]));

    typedef FloatRun<3>::vec_t float3v;
    unsigned int tag = 0;
    for (int it = cluster; it < n_units; it += n_clusters) {   // unit of work = NGRP consecutive groups
        const float *gp[2];
        float *op[2];
        bool wok[2];
        float hst[2];
        float3v gq[2][PF];
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            int win = (NGRP * it + x) * GW + wl;
            wok[x] = win < B;
            if (!wok[x]) win = B - 1;
            gp[x] = gid + ((size_t)win * T + t_first) * kGG + 3 * unit;
            op[x] = outd + ((size_t)win * T + t_first) * ldo + unit;
            hst[x] = 0.f;
        }
        __syncthreads();                                  // previous unit's images are dead
#pragma unroll
        for (int x = 0; x < 2; ++x) {                     // h_0 = 0
            uint32_t *z = reinterpret_cast<uint32_t *>(img[x][tag & 1]);
            for (int i = tid; i < kGImgBytes / 4; i += 512) z[i] = 0u;
        }
        auto refill = [&](int x, int p, bool advance) {
            gq[x][p] = load_run<3>(gp[x]);
            if (advance) gp[x] += gstride;
        };
#pragma unroll
        for (int x = 0; x < 2; ++x) {
#pragma unroll
            for (int p = 0; p < PF; ++p) gq[x][p] = float3v{0.f, 0.f, 0.f};
#pragma unroll
            for (int p = 0; p + 1 < PF; ++p) refill(x, p, p + 1 < T);
        }
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int p = 0; p + 1 < PF; ++p) {
                asm volatile("" ::"v"(gq[x][p].x)); asm volatile("" ::"v"(gq[x][p].y)); asm volatile("" ::"v"(gq[x][p].z));
            }
        __syncthreads();

        auto gather_issue = [&](int y, unsigned int gtag, uint4 (&v)[2]) {
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(ex + (size_t)(2 * y + (gtag & 1)) * kGGranules, 0,
                                                                kGGranules * 8, 0x00020000);
#pragma unroll
            for (int j = 0; j < 2; ++j)
                v[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (tid + 512 * j) * 16, 0, 16));
        };
        auto gather_finish = [&](int y, unsigned int gtag, uint4 (&v)[2]) {
            unsigned char *wb = img[y][gtag & 1];
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(ex + (size_t)(2 * y + (gtag & 1)) * kGGranules, 0,
                                                                kGGranules * 8, 0x00020000);
            int spins = 0;
            bool bad;
            do {
                bad = false;
#pragma unroll
                for (int j = 0; j < 2; ++j)
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
            for (int j = 0; j < 2; ++j) {
                *reinterpret_cast<unsigned int *>(wb + g_off[j]) = (v[j].x & 0xffffu) | (v[j].z << 16);
                *reinterpret_cast<unsigned int *>(wb + g_off[j] + 16) = (v[j].x >> 16) | (v[j].z & 0xffff0000u);
            }
        };
        auto half_step = [&](int x, int p, int step, bool do_gather, unsigned int gtag) {
            const unsigned char *rb = img[x][(tag - 1) & 1];
            uint4 v[2];
            if constexpr (NGRP == 2) { if (do_gather) gather_issue(1 - x, gtag, v); }
            if constexpr (NGRP == 2) refill(x, (p + PF - 1) % PF, (step + PF) < T);
            __builtin_amdgcn_sched_barrier(0);
            floatx4 acc0 = floatx4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#pragma unroll
            for (int ks = 0; ks < kGKS; ks += 2) {
                const half8 a0 = *reinterpret_cast<const half8 *>(rb + ks * kHKStride + rd_off);
                const half8 a1 = *reinterpret_cast<const half8 *>(rb + (ks + 1) * kHKStride + rd_off);
                acc0 = mfma16(wf[ks][0], a0, acc0);          // A = W (rows = gate rows), B = h (columns = windows)
                acc1 = mfma16(wf[ks + 1][0], a1, acc1);
                if constexpr (!HP) {
                    acc0 = mfma16(wf[ks][1], a0, acc0);
                    acc1 = mfma16(wf[ks + 1][1], a1, acc1);
                }
            }
            // acc[r] = gate r (r, z, n, 0) of unit g for column c; fp32-parity: add the lo column (lane c ^ 1)
            float pre[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                float dot = acc0[r] + acc1[r];
                if constexpr (!HP) dot += dpp_mov<0xB1>(dot);     // quad_perm:[1,0,3,2]
                pre[r] = dot;
            }
            const float3v gv = gq[x][p];
            const float rv = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((pre[0] + gv.x) * c_sig));
            const float zv = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((pre[1] + gv.y) * c_sig));
            const float na = __builtin_fmaf(rv, pre[2] + bhn, gv.z);
            const float nv = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(na * c_tanh)), 1.0f);
            const float h = __builtin_fmaf(zv, hst[x] - nv, nv);
            hst[x] = h;
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
            unsigned long long *dst = ex + (size_t)(2 * x + (tag & 1)) * kGGranules;
            if (!(c & 1)) {
                const unsigned long long gran = ((unsigned long long)tag << 32) | payload;
                if (same_xcd)
                    __hip_atomic_store(dst + (c >> 1) * kGH + unit, gran, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else
                    __hip_atomic_store(dst + (c >> 1) * kGH + unit, gran, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (lead && step < T && wok[x]) op[x][0] = h;
            op[x] += ostride;
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (NGRP == 1) {
                for (int i = 0; i < poll_delay; ++i) __builtin_amdgcn_s_sleep(1);
                gather_issue(x, gtag, v);
            }
            if (do_gather) gather_finish(NGRP == 2 ? 1 - x : x, gtag, v);
            if constexpr (NGRP == 1) refill(x, (p + PF - 1) % PF, (step + PF) < T);
            lds_barrier();
        };

        for (int step0 = 0; step0 < T; step0 += PF) {
#pragma unroll
            for (int p = 0; p < PF; ++p) {
                const int step = step0 + p;      // steps >= T run too (stores masked): all members agree
                ++tag;
                if constexpr (NGRP == 2) {
                    half_step(0, p, step, step > 0, tag - 1);
                    half_step(1, p, step, true, tag);
                } else {
                    half_step(0, p, step, true, tag);
                }
                if (s_abort[tag & 1]) {
                    if (tid == 0) atomicExch(status, 1);
                    return;
                }
            }
        }
        if constexpr (NGRP == 2) {   // B's last step: keeps "nobody publishes t+2 before everybody gathered t" across units
            uint4 v[2];
            gather_issue(1, tag, v);
            gather_finish(1, tag, v);
        }
        __syncthreads();
        if (s_abort[0] | s_abort[1]) {
            if (tid == 0) atomicExch(status, 1);
            return;
        }
    }
}

}  // namespace mdk
