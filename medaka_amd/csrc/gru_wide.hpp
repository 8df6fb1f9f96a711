// GRU(256): the consensus GRU at the width `medaka train` builds by default (reference medaka/models.py DEFAULT_MODEL_DICT:
// GRUModel(num_features=10, num_classes=5, gru_size=256)), on the cluster recurrence of cluster.hpp: 8 work-groups (= 8 CUs)
// per cluster, 64 VGPRs of W_hh fragments per lane (8 k-steps x hi/lo).  A unit's rows are (r, z, n, 0): the fourth is zero,
// so that the accumulator of lane (g, c) is exactly (r, z, n) of unit g for column c.  The grid is [8 XCDs x clusters / 8 x
// 8 members] x directions: both directions of a layer run in one launch, each direction its own clusters and exchange buffer.
// A time-out raises `status[0]`; the host re-runs the forward or reports MDK_ERR_DEVICE (gru_wide_run.hpp).
#pragma once
#include "cluster.hpp"

namespace mdk {

constexpr int kGH = 256;                        // hidden units
constexpr int kGG = 3 * kGH;                    // gi columns per direction (permuted: 3 * unit + gate)
constexpr int kGC = kGH / 32;                   // work-groups (CUs) per cluster
constexpr int kGKS = kGH / 32;                  // k-steps of the recurrent contraction

// Clusters of one launch: at most kGClusterBudget x 8 CUs for all directions of a process (`gpu_share` processes divide them), so
// that every member of every cluster can be resident at once on a GPU whose CUs the process shares with nothing else.
constexpr int kGClusterBudget = 28;     // 224 of 256 CUs
inline WidePlan plan_gru_wide(int nb, int D, bool hp, int gpu_share) {
    WidePlan w = plan_wide(nb, hp, kGC, std::max(1, std::min(kWMaxClusters, kGClusterBudget / (D * gpu_share))));
    w.work_groups *= D;                 // one launch for all directions
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

// n = tanh(gi_n + r * (W_hn h + b_hn)), h' = n + z (h - n): gi (input projection with b_ih, and b_hr / b_hz folded) arrives
// pre-scaled by S = kActScale * sw like the accumulator, b_hn is scaled here.
struct GruCell {
    static constexpr int H = kGH, GI = 3, NG = 3;
    typedef FloatRun<3>::vec_t gi_t;
    float c_sig, c_tanh, bhn;

    __device__ __forceinline__ gi_t load_gi(const float *p) const { return load_run<3>(p); }
    __device__ __forceinline__ float state0(bool, int) const { return 0.f; }
    __device__ __forceinline__ void image0(unsigned char *im, bool, int, long, const int (&)[2]) const {   // h_0 = 0
        zero_image<kGKS * kHKStride>(im);
    }
    __device__ __forceinline__ float step(const float (&pre)[3], gi_t gv, float &hst, bool) const {
        const float rv = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((pre[0] + gv.x) * c_sig));
        const float zv = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((pre[1] + gv.y) * c_sig));
        const float na = __builtin_fmaf(rv, pre[2] + bhn, gv.z);
        const float nv = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(na * c_tanh)), 1.0f);
        hst = __builtin_fmaf(zv, hst - nv, nv);
        return hst;
    }
    __device__ __forceinline__ void save(int, float) const {}
};

// The reverse direction scans T-1 .. 0 and writes column t.
template <int PF, int NGRP, bool HP = false>
__global__ __launch_bounds__(512, 1) void k_gru_wide(
    const float *__restrict__ gi,       // [D][B*T][768] permuted gate columns, biases folded, PRE-SCALED by S
    const half8 *__restrict__ wfrag,    // [D][8 members][8 waves][8 ks][2 hi/lo][64]
    const float *__restrict__ b_hn,     // [D][256] unscaled
    const float *__restrict__ inv_scale_d,   // [D] 1 / S
    float *__restrict__ out,            // [B*T][D*256]: direction d writes units d*256 ..
    unsigned long long *exch,           // [D][wide_exch_words(256)] granules + headers, zeroed before the launch
    int *status,                        // [0] != 0: a cluster timed out
    int B, int T, int D, int n_clusters, int n_units, int poll_delay, int skip_if_lost)
{
    const int dir = blockIdx.y;
    const ClusterSlot cs = cluster_slot<kGH>();
    if (cs.cluster >= n_clusters) return;
    if (skip_if_lost && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    unsigned long long *ex_dir = exch + (size_t)dir * wide_exch_words(kGH);
    const WideW<kGH, HP> w = load_wide_w<kGH, HP>(wfrag + (size_t)dir * kGC * 8 * (kGKS * 2) * 64, cs.member);
    const int placed = cluster_handshake<kGH>(ex_dir, cs.cluster, cs.member);
    if (placed < 0) return raise_status(status);
    constexpr float L2E = 1.44269504088896340736f;
    const float inv_scale = inv_scale_d[dir];
    const GruCell cell{-L2E * inv_scale, 2.0f * L2E * inv_scale, b_hn[dir * kGH + cluster_unit(cs.member)] * (1.0f / inv_scale)};
    cluster_scan<PF, NGRP, HP>(cell, w, ex_dir, status, placed == 1, cs,
                               n_clusters, n_units, gi + (size_t)dir * B * T * kGG, out + dir * kGH, D * kGH, B, T, dir, 0, T,
                               poll_delay);
}

}  // namespace mdk
