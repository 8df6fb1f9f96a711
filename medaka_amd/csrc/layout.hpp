// HBM layouts of the intermediates (DESIGN.md "data layout").
//
// Windows are grouped in tiles of 8.  Both intermediates are stored tile-major and, inside a
// (tile, t) block, in the register order of the recurrence kernel, so that every wave-level
// load/store of the serial kernel is one contiguous 256-byte run (the natural [window][t][f]
// layout made each of them four 64-byte runs 15 MB apart, and the kernel was bound by the number
// of cache lines its vector-memory instructions touched, not by bytes):
//
//   gi_t  [dir][tile][t][w8 8][q 2][lane 64][gate NG]  fp32   NG = 3 (GRU): 12 KB per block
//         (gate fastest: the recurrence reads the NG pre-activations of its (unit, window) with ONE 12- or
//          16-byte load per lane and the GEMM stores them with one: three dword loads 256 B apart cost 4.4 %
//          of the recurrence, profiles/r2_ablation.txt mask 32)
//   act_t [tile][t][dir][w8 8][q 2][lane 64]            fp32   D*1024 floats per block
//
// with  lane = g*16 + c,  window-in-tile = 2*g + q,  hidden unit = 16*w8 + c.
// Feature f of an activation row (f = dir*128 + unit) lives in chunk f>>4 = dir*8 + w8.
#pragma once
#include <stddef.h>

namespace mdk {

constexpr int kTileWin = 8;          // windows per tile
// NG = gate tiles per hidden unit: 3 for the GRU (r, z, n), 4 for the LSTM (i, f, g, o)
__host__ __device__ inline constexpr int gi_block_floats(int NG) { return 8 * 2 * NG * 64; }

__host__ __device__ inline size_t gi_block(int dir, int n_tiles, int tile, int T, int t, int NG) {
    return (((size_t)dir * n_tiles + tile) * T + t) * gi_block_floats(NG);
}
__host__ __device__ inline int gi_in_block(int w8, int q, int gate, int lane, int NG) {
    return ((w8 * 2 + q) * 64 + lane) * NG + gate;
}
__host__ __device__ inline size_t act_block(int D, int tile, int T, int t) {
    return ((size_t)tile * T + t) * (size_t)(D * 1024);
}
__host__ __device__ inline int act_in_block(int dir, int w8, int q, int lane) {
    return ((dir * 8 + w8) * 2 + q) * 64 + lane;
}

// Split scan (scan_split.hpp): a batch of B windows of T columns runs as S*B virtual windows of Tv columns.
constexpr int kMaxSplit = 16;
// SplitPlanCore is what every kernel of a split call takes by value; only the last layer's fused recurrence (rec_fused.hpp) and
// the host take the whole SplitPlan, with the scan ranges behind it.
struct SplitPlanCore {
    int S = 1;                    // chunks per window (1 = not split)
    int B = 0, T = 0;             // the real batch
    int Tv = 0;                   // columns of a virtual window
    int G = 0;                    // margin
    int start[kMaxSplit];         // first real column of chunk k
    int core0[kMaxSplit + 1];     // real columns [core0[k], core0[k+1]) are delivered from chunk k
};
struct SplitPlan : SplitPlanCore {
    // Scan range of the LAST layer inside chunk k's virtual window (gru_split.hpp plan_scan_ranges; local columns, multiples of
    // 8): the forward scan runs [lo_f, hi_f) upwards, the reverse scan [lo_r, hi_r) downwards, lo_f <= lo_r and hi_f <= hi_r.
    // Always filled and always read: the final-head scan of EVERY split call takes its steps from these arrays (gru_pass.hpp
    // layer_final_head_ranged, rec_fused.hpp `rng`); at trim = 0 they hold [0, Tv) for every chunk, which reproduces the layout a
    // split scan had before there were ranges -- cut at Tv/2, the same launches, the outer margin as the last one.
    int trim = 0;
    int lo_f[kMaxSplit], hi_f[kMaxSplit];
    int lo_r[kMaxSplit], hi_r[kMaxSplit];
};

// The last layer's scan range of one recurrence tile (8 consecutive virtual windows): the union over the chunks its windows
// belong to -- a tile that mixes chunks (B not a multiple of 8) runs the wider range, extra warm-up and extra trailing columns
// are harmless -- and the midpoint at which the scan is cut into its two halves.  The first half runs forward over [lo_f, mid)
// and reverse over [mid, hi_r), the second forward over [mid, hi_f) and reverse over [lo_r, mid): what the second half finishes
// lies inside what the other direction covered in the first.  Both direction work-groups of a tile, and the host, get the same.
struct ScanRange { int lo_f, hi_f, lo_r, hi_r, mid; };
__host__ __device__ inline int split_mid(int lo, int hi) { return (lo + hi) / 2 / 8 * 8; }
__host__ __device__ inline ScanRange split_tile_range(const SplitPlan &p, int tile, int nb) {
    const int w0 = tile * kTileWin, w1 = w0 + kTileWin - 1 < nb ? w0 + kTileWin - 1 : nb - 1;
    const int k0 = w0 / p.B, k1 = w1 / p.B;
    ScanRange r{p.lo_f[k0], p.hi_f[k0], p.lo_r[k0], p.hi_r[k0], 0};
    for (int k = k0 + 1; k <= k1; ++k) {
        r.lo_f = p.lo_f[k] < r.lo_f ? p.lo_f[k] : r.lo_f;
        r.hi_f = p.hi_f[k] > r.hi_f ? p.hi_f[k] : r.hi_f;
        r.lo_r = p.lo_r[k] < r.lo_r ? p.lo_r[k] : r.lo_r;
        r.hi_r = p.hi_r[k] > r.hi_r ? p.hi_r[k] : r.hi_r;
    }
    r.mid = split_mid(r.lo_f, r.hi_r);
    return r;
}

}  // namespace mdk
