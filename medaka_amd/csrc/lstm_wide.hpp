// LSTM(384) of the bundled read-level models (`rl_lstm384`: LatentSpaceLSTM(lstm_size=384,
// cnn_size=128, bidirectional=False), reference medaka/architectures/latent_space_lstm.py:129-149),
// on the cluster recurrence of cluster.hpp: 12 work-groups (= 12 CUs) per cluster, 96 VGPRs of
// W_hh fragments per lane (12 k-steps x hi/lo), the accumulator of lane (g, c) holds (i, f, g, o)
// of unit g for window c.  The grid is 8 XCDs x 2 clusters x 12 members = 192 work-groups <= 256 CUs.
#pragma once
#include "cluster.hpp"

namespace mdk {

constexpr int kWH = 384;                       // hidden units
constexpr int kWG4 = 4 * kWH;                  // gate columns
constexpr int kWC = kWH / 32;                  // work-groups (CUs) per cluster
constexpr int kWKS = kWH / 32;                 // k-steps of the recurrent contraction

// c' = f c + i g, h = o tanh(c'): gi arrives pre-scaled by S like the accumulator.  The scan may run as several launches
// (scan steps [s0, s0 + ns)): a launch with s0 > 0 resumes from the h it stored at scan step s0 - 1 and the cell state in
// cstate, which every launch leaves behind.
template <bool HP>
struct LstmCell {
    static constexpr int H = kWH, GI = 4, NG = 4;
    typedef floatx4 gi_t;
    const float *out;
    float *cstate;
    int B, T, s0, unit;
    float c_sig, c_tanh;

    __device__ __forceinline__ gi_t load_gi(const float *p) const { return *reinterpret_cast<const floatx4 *>(p); }
    __device__ __forceinline__ float state0(bool live, int win) const {
        return (s0 > 0 && live) ? cstate[(size_t)win * kWH + unit] : 0.f;
    }
    __device__ __forceinline__ void image0(unsigned char *im, bool live, int win0, long tprev, const int (&g_off)[3]) const {
        if (s0 == 0 || !live) {
            zero_image<kWKS * kHKStride>(im);
            return;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int gidx = 2 * (threadIdx.x + 512 * j);
            const int w = gidx / kWH, u = gidx % kWH;      // image rows 2w, 2w + 1; units u, u + 1
            auto row_of = [&](int wi) {
                int win = win0 + wi;
                if (win >= B) win = B - 1;
                return out + ((size_t)win * T + tprev) * kWH + u;
            };
            unsigned int r0, r1;
            if constexpr (HP) {      // rows = windows 2w, 2w + 1
                const float2 a = *reinterpret_cast<const float2 *>(row_of(2 * w));
                const float2 b2 = *reinterpret_cast<const float2 *>(row_of(2 * w + 1));
                r0 = (unsigned int)__builtin_bit_cast(unsigned short, (_Float16)(a.x * kActScale)) |
                     ((unsigned int)__builtin_bit_cast(unsigned short, (_Float16)(a.y * kActScale)) << 16);
                r1 = (unsigned int)__builtin_bit_cast(unsigned short, (_Float16)(b2.x * kActScale)) |
                     ((unsigned int)__builtin_bit_cast(unsigned short, (_Float16)(b2.y * kActScale)) << 16);
            } else {                 // rows = (window w, hi), (window w, lo)
                const float2 a = *reinterpret_cast<const float2 *>(row_of(w));
                _Float16 h0, l0, h1, l1;
                split_f16(a.x * kActScale, h0, l0);
                split_f16(a.y * kActScale, h1, l1);
                r0 = (unsigned int)__builtin_bit_cast(unsigned short, h0) | ((unsigned int)__builtin_bit_cast(unsigned short, h1) << 16);
                r1 = (unsigned int)__builtin_bit_cast(unsigned short, l0) | ((unsigned int)__builtin_bit_cast(unsigned short, l1) << 16);
            }
            *reinterpret_cast<unsigned int *>(im + g_off[j]) = r0;
            *reinterpret_cast<unsigned int *>(im + g_off[j] + 16) = r1;
        }
    }
    __device__ __forceinline__ float step(const float (&pre)[4], gi_t gv4, float &cst, bool live) const {
        constexpr float L2E = 1.44269504088896340736f;
        const float iv = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((pre[0] + gv4.x) * c_sig));
        const float fv = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((pre[1] + gv4.y) * c_sig));
        const float gg = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((pre[2] + gv4.z) * c_tanh)), 1.0f);
        const float ov = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((pre[3] + gv4.w) * c_sig));
        const float cv = __builtin_fmaf(fv, cst, iv * gg);
        if (live) cst = cv;        // (padding steps must not disturb the state a later launch resumes from)
        const float tc = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(cv * (2.0f * L2E))), 1.0f);
        return ov * tc;
    }
    __device__ __forceinline__ void save(int win, float cst) const { cstate[(size_t)win * kWH + unit] = cst; }
};

template <int PF, int NGRP, bool HP = false>
__global__ __launch_bounds__(512, 1) void k_lstm_wide(
    const float *__restrict__ gi,       // [B*T][1536] permuted gate columns, bias folded, PRE-SCALED by S
    const half8 *__restrict__ wfrag,    // [12 members][8 waves][12 ks][2 hi/lo][64]
    float *__restrict__ out,            // [B*T][384]
    unsigned long long *exch,           // [wide_exch_words(384)] granules + headers, zeroed
    int *status,                        // [0] != 0: a cluster timed out
    int B, int T, int reverse, float inv_scale, int n_clusters, int n_units, int force_wt, int poll_delay,
    int s0, int ns, float *__restrict__ cstate,   // scan steps [s0, s0 + ns); cell state [B][384] between launches
    int skip_if_lost)                             // synchronous forwards: return at once when status[0] is already up
{
    const ClusterSlot cs = cluster_slot<kWH>();
    if (cs.cluster >= n_clusters) return;
    // a cluster of an EARLIER launch of this forward timed out: the forward is lost and will be re-run or reported;
    // do not spend another handshake time-out on each of its remaining launches.  (Not in asynchronous mode, where
    // the flag of an earlier forward stays up until the caller asks with mdk_rl_check: later forwards must still run.)
    if (skip_if_lost && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    const WideW<kWH, HP> w = load_wide_w<kWH, HP>(wfrag, cs.member);
    const int placed = cluster_handshake<kWH>(exch, cs.cluster, cs.member);
    if (placed < 0) return raise_status(status);
    constexpr float L2E = 1.44269504088896340736f;
    const LstmCell<HP> cell{out, cstate, B, T, s0, cluster_unit(cs.member), -L2E * inv_scale, 2.0f * L2E * inv_scale};
    cluster_scan<PF, NGRP, HP>(cell, w, exch, status, placed == 1 && !force_wt, cs, n_clusters, n_units, gi, out, kWH,
                               B, T, reverse, s0, s0 + ns, poll_delay);
}

}  // namespace mdk
