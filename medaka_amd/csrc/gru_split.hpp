// The split scan on the host side: shape arithmetic, enqueue / finish halves of a split call, the two forwards that run it -- the
// synchronous one (run_forward: wait, certificate, retries, audit, fallback) with the first attempt of a call started ahead
// (start_call), and the stream-ordered one (enqueue_async, retire_one).  What a call's verdict teaches the model is SplitPolicy's
// (split_policy.hpp), for both.  Part of api.hip (included there after gru_pass.hpp).
#pragma once
// ---- split scan (scan_split.hpp): plan, run on the virtual batch, certify, fall back
// The shape arithmetic of a split, free of any model state (also exported as mdk_split_plan for hosts and CPU tests).
//   mode: 1 auto, n >= 2 forced chunk count; share: processes on this GPU; G: margin; budget: column budget of a pass
static void plan_scan_ranges(SplitPlan &p, int trim);
static bool plan_split_shape(int B, int T, int share, int mode, int G, size_t budget, SplitPlan &p) {
    p.S = 1; p.B = B; p.T = T; p.Tv = T; p.G = 0; p.trim = 0;
    if (B < 1 || T < 1 || mode < 1 || G < 8 || share < 1) return false;
    // The recurrence holds 8 windows per work-group and direction at most (fp32-parity mode): 1024 chunk-windows are
    // one round of work-groups on 256 CUs -- more than that queues (profiles/r3_experiments/scan_split/time_probe.txt).
    // K processes sharing the GPU (launch.py --procs-per-gpu): their kernels interleave -- one is in its projection
    // while another is in a recurrence -- and 1600 / K chunk-windows each measured best (profiles/r3_fed_loop_shared.txt:
    // K = 3 at batch 200, whole fed loop: 249 M columns/s unsplit, 290 M with 2 chunks, 284 M with 3)
    const int max_win = share == 1 ? 1024 : 1600 / share;
    int S = (mode >= 2) ? mode : max_win / B;
    // alone, two chunks of 500 windows gain 8 % on the device and nothing host to host: not worth the margins
    if (mode == 1 && S < (share == 1 ? 3 : 2)) return false;
    S = std::min({S, kMaxSplit, T / (4 * G)});      // a chunk's own columns are at least twice its two margins
    if (S < 2) return false;
    int max_core = 0, core0[kMaxSplit + 1];
    for (int k = 0; k <= S; ++k) core0[k] = (int)((long)T * k / S);
    for (int k = 0; k < S; ++k) max_core = std::max(max_core, core0[k + 1] - core0[k]);
    const int Tv = (max_core + 2 * G + 15) / 16 * 16;
    if (Tv >= T || (size_t)S * B * Tv > budget) return false;
    p.S = S; p.G = G; p.Tv = Tv;
    for (int k = 0; k <= S; ++k) p.core0[k] = core0[k];
    for (int k = 0; k < S; ++k) p.start[k] = std::min(std::max(core0[k] - G, 0), T - Tv);
    plan_scan_ranges(p, 0);
    return true;
}

// What the LAST layer scans of every chunk (option "scan_split_trim").  A chunk is run over its core plus G
// columns on either side, but past its core, in scan order, the only reader of the last layer's state is the certificate's second
// point, G/2 columns past the junction (scan_split.hpp k_split_verify): no head output comes from the G/2 columns behind it
// (rec_fused.hpp FinRow clips to the core), no later layer exists and no certificate point lies there.  And before its core the
// last layer is fed, for its first G/2 columns, by a previous layer that is itself still warming up.  In real columns:
//   forward:  [k == 0 ? 0 : core0[k] - lead,   k == S-1 ? T : core0[k+1] + G/2)   upwards
//   reverse:  [k == 0 ? 0 : core0[k] - G/2,    k == S-1 ? T : core0[k+1] + lead)  downwards
//   trim 0: the whole virtual window;  1: lead = G, the trailing half-margin goes;  2: lead = G/2, the leading one as well
// made local (- start[k]) and rounded outwards to the strip of the fused recurrence (8 columns; Tv is a multiple of 16), so that
// the four launch lengths around any midpoint that is a multiple of 8 are whole strips (layout.hpp split_tile_range).
// Level 1 vs level 0: interior chunks compute the same states from the same inputs.  An edge chunk's window is shifted inwards --
// 2 G of lead, of which its scan now skips the first G, so its junction is warmed over G columns like every other -- and its
// states differ until the two trajectories have merged.  Where the certificate holds they have, to the last bit, long before
// the first delivered column: certified calls deliver level 0's bits on all seven weight sets (tests/test_split_trim_gpu.py,
// profiles/l1_scan_range/README.md); that is measured, not guaranteed, and the junction difference of a REJECTED call differs
// in its last digits.  Level 2 changes results at the rounding-noise level, and a model with a long memory needs the next larger
// margin with it (`hp`: 256 instead of 192): the default is 1.
static void plan_scan_ranges(SplitPlan &p, int trim) {
    p.trim = p.S > 1 ? std::min(std::max(trim, 0), 2) : 0;
    for (int k = 0; k < kMaxSplit; ++k) { p.lo_f[k] = p.lo_r[k] = 0; p.hi_f[k] = p.hi_r[k] = p.Tv; }
    if (!p.trim) return;
    const int half = p.G / 2, lead = p.trim >= 2 ? half : p.G;
    auto down = [&](int t, int k) { return std::max(0, (t - p.start[k]) & ~7); };
    auto up = [&](int t, int k) { return std::min(p.Tv, (t - p.start[k] + 7) & ~7); };
    for (int k = 0; k < p.S; ++k) {
        p.lo_f[k] = k == 0 ? 0 : down(p.core0[k] - lead, k);
        p.lo_r[k] = k == 0 ? 0 : down(p.core0[k] - half, k);
        p.hi_f[k] = k == p.S - 1 ? p.Tv : up(p.core0[k + 1] + half, k);
        p.hi_r[k] = k == p.S - 1 ? p.Tv : up(p.core0[k + 1] + lead, k);
    }
}

// The margin learner on a model that certifies iff the margin is >= `need` (0: never), with differences at the noise floor:
// n_calls calls from `start`; margins[i] = the margin call i was ANSWERED at (0: sequentially), forwards[i] = split forwards
// it cost (rejected ones included).  Device-free: the CPU tests drive SplitPolicy's verdicts through this, as run_forward does
// (fp32, auto mode); after a give-up every later call is answered sequentially (the back-off is not counted down here).
extern "C" int mdk_margin_sim(int start, int adapt, int need, int n_calls, int *margins, int *forwards) {
    if (start < 16 || start > 4096 || adapt < 0 || need < 0 || n_calls < 0 || !margins || !forwards)
        return fail(MDK_ERR_ARG, "bad argument");
    SplitPolicy P;
    P.opt_scan_split = 1; P.opt_split_margin = start; P.opt_split_adapt = adapt;
    for (int i = 0; i < n_calls; ++i) {
        margins[i] = 0; forwards[i] = 0;
        if (P.split_disabled) continue;
        for (;;) {
            const int G = P.margin_in_use();
            forwards[i]++;
            if (need > 0 && G >= need) { P.certified(G, MDK_PREC_FP32, true); margins[i] = G; break; }
            if (!P.rejected(G, true)) break;
        }
    }
    return MDK_OK;
}

// plan_pass on a model that exists on paper only (default options): nothing here touches a device
extern "C" int mdk_pass_plan(const mdk_gru_desc *desc, int precision, int gpu_share, int windows, int T, int host_io, int split_chunks,
                             int mode, mdk_pass_shape *out) {
    if (!desc || !out) return fail(MDK_ERR_ARG, "null argument");
    if (windows < 1 || T < 1 || gpu_share < 1 || gpu_share > 8 || split_chunks < 0 || split_chunks > kMaxSplit ||
        (precision != MDK_PREC_FP32 && precision != MDK_PREC_FP16) || desc->num_layers < 1 || desc->num_features < 1 ||
        (desc->hidden != kH && desc->hidden != kGH))
        return fail(MDK_ERR_ARG, "bad argument (windows=%d T=%d gpu_share=%d split_chunks=%d precision=%d hidden=%d; hidden 128 or 256)",
                    windows, T, gpu_share, split_chunks, precision, desc->hidden);
    mdk_gru m;
    m.desc = *desc;
    m.D = desc->bidirectional ? 2 : 1;
    m.precision = precision;
    m.opt_gpu_share = gpu_share;
    m.oor_seen = (mode & 4) != 0;
    m.layers.resize((size_t)desc->num_layers);
    m.layers[0].K = desc->num_features;
    // (the fused layer-0 projection exists when the features + the bias row fit one 16-slot k-group: mdk_gru_create)
    m.layers[0].wx_frag = desc->num_features + 1 <= 16 ? reinterpret_cast<half8 *>(sizeof(half8)) : nullptr;
    static const float dummy = 0.f;
    HostIO io;
    if (host_io & 1) io.x_host = &dummy;
    if (host_io & 2) io.p_host = const_cast<float *>(&dummy);
    SplitPlan sp;
    sp.S = split_chunks;
    PassPlan P;
    const int rc = plan_pass(&m, windows, T, (host_io & 3) ? &io : nullptr, split_chunks > 1 ? &sp : nullptr, P, (mode & 1) != 0, (mode & 2) != 0,
                             (mode & 8) != 0);
    if (rc) return rc;
    memset(out, 0, sizeof(*out));
    out->windows_per_group = 4 * P.nq; out->work_groups = P.n_wg;
    out->fuse_layer0 = P.fuse0; out->fuse_projection = P.fuse_proj; out->fuse_head = P.fuse_head; out->final_head = P.final_head;
    out->overlap_gemm = P.overlap; out->stream_in = P.stream_in; out->stream_out = P.stream_out;
    out->needs_gi = P.need_gi;
    return MDK_OK;
}

extern "C" int mdk_split_plan(int B, int T, int gpu_share, int scan_split, int margin, mdk_split_shape *out) {
    if (!out) return fail(MDK_ERR_ARG, "null argument");
    if (B < 0 || T < 0 || gpu_share < 1 || gpu_share > 8 || scan_split < 0 || scan_split > kMaxSplit || margin < 16 || margin > 4096 || margin % 8)
        return fail(MDK_ERR_ARG, "bad argument (B=%d T=%d gpu_share=%d scan_split=%d margin=%d)", B, T, gpu_share, scan_split, margin);
    SplitPlan p;
    plan_split_shape(B, T, gpu_share, scan_split, margin, kMaxRowsPerPass, p);
    memset(out, 0, sizeof(*out));
    out->chunks = p.S; out->columns = p.S > 1 ? p.Tv : T; out->margin = p.S > 1 ? p.G : 0;
    for (int k = 0; k < p.S && p.S > 1; ++k) { out->start[k] = p.start[k]; out->first[k] = p.core0[k]; out->last[k] = p.core0[k + 1]; }
    if (p.S == 1) { out->start[0] = 0; out->first[0] = 0; out->last[0] = T; }
    return MDK_OK;
}

extern "C" int mdk_split_scan_ranges(int B, int T, int gpu_share, int scan_split, int margin, int trim, mdk_split_ranges *out) {
    if (!out) return fail(MDK_ERR_ARG, "null argument");
    if (B < 0 || T < 0 || gpu_share < 1 || gpu_share > 8 || scan_split < 0 || scan_split > kMaxSplit || margin < 16 || margin > 4096 || margin % 8 ||
        trim < 0 || trim > 2)
        return fail(MDK_ERR_ARG, "bad argument (B=%d T=%d gpu_share=%d scan_split=%d margin=%d trim=%d)", B, T, gpu_share, scan_split, margin, trim);
    SplitPlan p;
    plan_split_shape(B, T, gpu_share, scan_split, margin, kMaxRowsPerPass, p);
    plan_scan_ranges(p, trim);
    memset(out, 0, sizeof(*out));
    out->chunks = p.S; out->trim = p.trim;
    for (int k = 0; k < p.S; ++k) {
        out->lo_fwd[k] = p.lo_f[k]; out->hi_fwd[k] = p.hi_f[k]; out->lo_rev[k] = p.lo_r[k]; out->hi_rev[k] = p.hi_r[k];
        out->mid[k] = split_mid(p.lo_f[k], p.hi_r[k]);
    }
    return MDK_OK;
}

extern "C" int mdk_split_tile_ranges(int B, int T, int gpu_share, int scan_split, int margin, int trim, int max_tiles, int *n_tiles, int *out) {
    if (!n_tiles || (max_tiles > 0 && !out)) return fail(MDK_ERR_ARG, "null argument");
    if (B < 1 || T < 1 || gpu_share < 1 || gpu_share > 8 || scan_split < 0 || scan_split > kMaxSplit || margin < 16 || margin > 4096 || margin % 8 ||
        trim < 0 || trim > 2 || max_tiles < 0)
        return fail(MDK_ERR_ARG, "bad argument (B=%d T=%d gpu_share=%d scan_split=%d margin=%d trim=%d)", B, T, gpu_share, scan_split, margin, trim);
    SplitPlan p;
    plan_split_shape(B, T, gpu_share, scan_split, margin, kMaxRowsPerPass, p);
    plan_scan_ranges(p, trim);
    const int nb = p.S * p.B;
    *n_tiles = (nb + kTileWin - 1) / kTileWin;
    for (int t = 0; t < *n_tiles && t < max_tiles; ++t) {
        const ScanRange r = split_tile_range(p, t, nb);      // (what k_rec_fused and layer_final_head_ranged compute)
        out[5 * t] = r.lo_f; out[5 * t + 1] = r.hi_f; out[5 * t + 2] = r.lo_r; out[5 * t + 3] = r.hi_r; out[5 * t + 4] = r.mid;
    }
    return MDK_OK;
}

static bool plan_split(const mdk_gru *m, int B, int T, SplitPlan &p) {
    static const int env_abl = getenv("MDK_ABLATE") ? atoi(getenv("MDK_ABLATE")) : 0;
    p.S = 1;
    const SplitPolicy &P = m->policy;
    if (P.opt_scan_split == 0 || (P.split_disabled && P.opt_scan_split == 1)) return false;
    if (m->wide) return false;             // GRU(256): sequential scans only
    if (m->variant != MDK_VARIANT_MFMA || m->D != 2 || m->desc.num_layers != 2 || m->opt_ablate || env_abl) return false;
    if (m->layers[0].K > 16) return false;
    if (!plan_split_shape(B, T, m->opt_gpu_share, P.opt_scan_split, P.margin_in_use(), m->max_rows_per_pass ? m->max_rows_per_pass : kMaxRowsPerPass, p))
        return false;
    plan_scan_ranges(p, m->opt_split_trim);
    return true;
}

// A split call in two halves, so that the staged entry can enqueue the NEXT batch's forward before it waits for this one's
// certificate: split_enqueue = every launch and copy of the call (nothing here waits for the device), split_finish = the wait,
// the range flag, the certificate.  run_split = one after the other.
// `dflag` (the stream-ordered entry): the certificate goes to these device words and stays there -- nothing is copied home, and the
// range decision is the device's (gi and the fallback launches are planned in)
static int split_enqueue(mdk_gru *m, const SplitPlan &sp, const float *x_dev, float *probs_dev, hipStream_t s,
                         const float *x_host, float *probs_host, EvTimer &tm, bool *need_gi, unsigned *dflag = nullptr) {
    const size_t F = m->desc.num_features;
    const int Bv = sp.S * sp.B;
    const size_t cols = (size_t)Bv * sp.Tv;
    memset(&m->last, 0, sizeof(m->last));
    m->last.n_layers = m->desc.num_layers;
    if (cols * F > m->xv_cap) {
        free_dev(m->xv); m->xv = nullptr; m->xv_cap = 0;
        HIP_TRY(hipMalloc((void **)&m->xv, cols * F * sizeof(float)));
        m->xv_cap = cols * F;
    }
    if (!m->split_flag) HIP_TRY(hipMalloc((void **)&m->split_flag, kSplitFlagWords * sizeof(unsigned)));
    if (!m->split_host) HIP_TRY(hipHostMalloc((void **)&m->split_host, kSplitFlagWords * sizeof(unsigned), hipHostMallocDefault));
    if (!m->oor_host) HIP_TRY(hipHostMalloc((void **)&m->oor_host, sizeof(int), hipHostMallocDefault));
    HostIO io;
    io.p_host = probs_host;
    if (probs_host && probs_host == m->tail_host) io.p_host_dev = m->tail_dev;      // (the cold host entry: the last chunks may leave by kernel)
    PassPlan P;                    // this call synchronises for its certificate anyway: it looks at the range flag itself
    int rc = plan_pass(m, Bv, sp.Tv, probs_host ? &io : nullptr, &sp, P, /*host_checks_range=*/dflag == nullptr);
    if (rc) return rc;
    *need_gi = P.need_gi;
    if ((rc = ensure_workspace(m, (((size_t)Bv + kTileWin - 1) / kTileWin * kTileWin) * (size_t)sp.Tv, P.need_gi))) return rc;
    static const bool dbg_spans = getenv("MDK_EARLY_DEBUG") != nullptr;
    if (dbg_spans) {
        hipEvent_t a, b;
        HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b));
        HIP_TRY(hipEventRecord(a, s));
        m->dbg_spans.push_back({a, b});
    }
    unsigned *flag = dflag ? dflag : m->split_flag;
    HIP_TRY(hipMemsetAsync(flag, 0, kSplitFlagWords * sizeof(unsigned), s));
    // Host buffers.  x crosses PCIe whole, one contiguous copy in front of the forward: all of it is needed within the
    // first half of layer 0 (1 ms of work against 1.4 ms of PCIe), so slabs gain nothing -- measured both as DMA slabs and
    // as copy kernels on the mapped buffer (profiles/r4_experiments/README.md); callers that can, hand x over early
    // (medaka_amd.torch_ext: the batch is on its way to the device while the previous one is still being computed).
    // The probabilities leave in column chunks, as 2-D DMA copies under the rest of the last layer's scan, whose second
    // half writes them itself (rec_fused.hpp HEAD = 2; forward_pass decides: `host_streamed` bit 1) -- behind a separate
    // head kernel they did not (a kernel beside a recurrence that holds every CU crawls until the recurrence is over: 9.4 ms
    // against 9.1, profiles/r4_experiments/host_path_timeline_v4_dma_out.txt; "stream_host" = 2 still forces that form).
    // What stays exposed is the last launch's chunk; a shape that cannot be chunked leaves as one copy behind the forward.
    if (x_host)
        HIP_TRY(hipMemcpyAsync(const_cast<float *>(x_dev), x_host, (size_t)sp.B * sp.T * F * sizeof(float), hipMemcpyHostToDevice, s));
    std::vector<hipEvent_t> out_done;      // (the last result chunks are still crossing PCIe while the certificate is computed)
    // (x_dev is the REAL batch: layer 0's operands are packed straight from it, chunk by chunk; m->xv -- the virtual batch in
    // memory -- is written only if the exact-projection fallback needs it)
    rc = forward_pass(m, P, x_dev, probs_dev, s, tm, probs_host ? &io : nullptr, &sp, &out_done);
    if (rc) return rc;
    hipLaunchKernelGGL(k_split_verify, dim3((unsigned)((sp.B + kVerifyWin - 1) / kVerifyWin), (unsigned)(8 * (sp.S - 1))), dim3(128), 0, s,
                       (const float *)m->act[0], (const float *)m->act[1], sp, flag);
    if (!dflag) HIP_TRY(hipMemcpyAsync(m->split_host, m->split_flag, kSplitFlagWords * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    // (no gi, hence no device-side fallback in this pass: the range flag goes home with the certificate)
    if (!P.need_gi) HIP_TRY(hipMemcpyAsync(m->oor_host, m->oor_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(m->kernels_done, s));        // the call's last kernel: the other context's next forward may start behind it
    if (dbg_spans) HIP_TRY(hipEventRecord(m->dbg_spans.back().second, s));
    for (hipEvent_t e : out_done) HIP_TRY(hipStreamWaitEvent(s, e, 0));
    HIP_TRY(hipGetLastError());
    return MDK_OK;
}

static int run_split(mdk_gru *m, const SplitPlan &sp, const float *x_dev, float *probs_dev, hipStream_t s,
                     const float *x_host, float *probs_host, bool *certified);

static int split_finish(mdk_gru *m, const SplitPlan &sp, bool need_gi, EvTimer &tm, const float *x_dev, float *probs_dev, hipStream_t s,
                        float *probs_host, bool *certified) {
    int rc;
    if ((rc = finish_timing(m, tm, s))) return rc;
    HIP_TRY(hipStreamSynchronize(s));      // the certificate decides what this call returns
    if (!need_gi && *m->oor_host != 0) {
        // the input left the fp16 range and nothing was there to take over: the model is marked and the call repeated, with gi
        // and the device-side decision, which later calls keep
        if (!m->oor_seen) {
            m->oor_seen = true;
            fprintf(stderr, "[medaka_amd] input beyond fp16 range (un-normalised counts?): the exact fp32 projection takes over -- this call is "
                            "repeated, later ones decide on the device\n");
        }
        return run_split(m, sp, x_dev, probs_dev, s, nullptr, probs_host, certified);
    }
    const float eps = m->precision == MDK_PREC_FP16 ? kSplitEpsHalf : kSplitEps;
    float worst = 0.f;
    for (int y = 0; y < 8 * (sp.S - 1); ++y) {
        float d;
        memcpy(&d, &m->split_host[y], sizeof(float));
        worst = std::max(worst, d);
    }
    *certified = worst <= eps;
    static const bool dbg = getenv("MDK_SPLIT_DEBUG") != nullptr;
    if (dbg) {
        fprintf(stderr, "[mdk split] %d x %d as %d chunks of %d columns (margin %d): %s, worst %.3g\n", sp.B, sp.T, sp.S, sp.Tv, sp.G,
                *certified ? "certified" : "REJECTED", worst);
        for (int y = 0; y < 8 * (sp.S - 1); ++y) {
            float d;
            memcpy(&d, &m->split_host[y], sizeof(float));
            fprintf(stderr, "    junction %d (column %d) layer %d direction %d point %d: %.3g\n", y >> 3, sp.core0[(y >> 3) + 1], (y >> 2) & 1,
                    (y >> 1) & 1, y & 1, d);
        }
    }
    m->policy.record(sp.S, sp.G, sp.Tv, worst, *certified);
    return MDK_OK;
}

static int run_split(mdk_gru *m, const SplitPlan &sp, const float *x_dev, float *probs_dev, hipStream_t s,
                     const float *x_host, float *probs_host, bool *certified) {
    EvTimer tm{m, s};
    bool need_gi = true;
    int rc = split_enqueue(m, sp, x_dev, probs_dev, s, x_host, probs_host, tm, &need_gi);
    if (rc) return rc;
    return split_finish(m, sp, need_gi, tm, x_dev, probs_dev, s, probs_host, certified);
}

// the buffer of an audit's sequential scan (n floats)
static int ensure_audit(mdk_gru *m, size_t n) {
    if (n > m->audit_cap) {
        free_dev(m->audit); m->audit = nullptr; m->audit_cap = 0;
        HIP_TRY(hipMalloc((void **)&m->audit, n * sizeof(float)));
        m->audit_cap = n;
    }
    return MDK_OK;
}

// one call: split scan when the shape is latency-bound and the certificate holds, the sequential passes otherwise
// `pre` (staged entry only): the call's FIRST attempt is already enqueued on `s` in this context (start_call) -- a split scan whose
// certificate is still unread, or the sequential passes.  It is taken over if it is what this function would have enqueued now;
// otherwise (an option, the learner or the back-off moved in between) it is waited for and forgotten.
static bool same_split(const SplitPlan &a, const SplitPlan &b) {
    if (a.S != b.S || a.B != b.B || a.T != b.T || a.Tv != b.Tv || a.G != b.G || a.trim != b.trim) return false;
    for (int k = 0; k < a.S; ++k) if (a.start[k] != b.start[k] || a.core0[k] != b.core0[k]) return false;
    return a.core0[a.S] == b.core0[b.S];
}

static int run_forward(mdk_gru *m, const float *x_dev, int B, int T, float *probs_dev, hipStream_t s,
                       const float *x_host, float *probs_host, mdk_gru::Started *pre = nullptr) {
    SplitPolicy &P = m->policy;
    SplitPlan sp;
    int rc;
    bool first_attempt = true;
    auto forget_pre = [&]() -> int {
        if (pre && pre->valid) {
            pre->valid = false;
            m->early_dropped++;
            HIP_TRY(hipStreamSynchronize(s));       // (its result copies target the caller's buffer: nothing of it may still be running)
        }
        return MDK_OK;
    };
    P.open_record(T, P.begin_call());
#ifdef MDK_DEBUG_HOOKS
    static const bool keep = getenv("MDK_SPLIT_KEEP") != nullptr;   // debug builds only: deliver a rejected split as it is
#else
    const bool keep = false;
#endif
    while (plan_split(m, B, T, sp)) {
        bool ok = false;
        // Half precision (what `medaka inference` runs by default, prediction.py:164-168).  Its certificate compares the fp16
        // images the scan keeps of h: two merged scans still differ by 1e-4 .. 3e-4 of rounding noise there, the threshold is
        // 2^-10, and a state that has NOT merged by up to 1e-3 passes unseen -- the margin learner then walks down to margins the
        // fp32-parity certificate rejects for the same weights (round 5: 64 where fp32 parity needs 128).  So in auto mode a margin
        // is used in half mode only after a call certified at it in FP32-PARITY mode: the call is run once more with the hi/lo
        // operands and the 2^-18 threshold (result discarded, x stays on the device), once per margin the learner visits and again
        // with every standing audit; a rejected probe is a rejected certificate (the margin climbs / the trial goes back).
        const bool probe_due = P.probe_due(sp.G, m->precision);
        const bool use_pre = first_attempt && pre && pre->valid && pre->split && pre->precision == m->precision && !probe_due &&
                             same_split(sp, pre->sp);
        if (first_attempt && !use_pre && (rc = forget_pre())) return rc;
        first_attempt = false;
        bool probe_rejected = false;
        if (probe_due) {
            m->precision = MDK_PREC_FP32;
            bool pok = false;
            rc = run_split(m, sp, x_dev, probs_dev, s, x_host, nullptr, &pok);
            m->precision = MDK_PREC_FP16;
            if (rc) return rc;
            x_host = nullptr;                     // x is on the device from here on
            P.probed(sp.G, pok, P.last_split.max_delta);
            probe_rejected = !pok;
        }
        if (!probe_rejected) {
            if (use_pre) {
                pre->valid = false;
                m->early_used++;
                EvTimer none{m, s};
                rc = split_finish(m, sp, pre->need_gi, none, x_dev, probs_dev, s, probs_host, &ok);
            } else {
                rc = run_split(m, sp, x_dev, probs_dev, s, x_host, probs_host, &ok);
            }
            if (rc) return rc;
        }
        if (keep) return MDK_OK;
        if (!ok) {
            if (P.rejected(sp.G, true)) continue;
            break;
        }
        P.certified(sp.G, m->precision, true);
        if (!P.audit_due(sp.G, m->precision)) return MDK_OK;
        const size_t n = (size_t)B * T * m->desc.num_classes;
        if ((rc = ensure_audit(m, n))) return rc;
        // (x_dev holds x also on the host path.)  The audit's scan is planned `lean`: it needs no gi -- 6 GB per buffer at
        // 200 x 10 000, which an audit used to allocate and give back: memory handed back to the driver is wiped by the
        // kernel ON THE DMA ENGINES, in the background, and while that ran (0.45 s for the two buffers) every strided copy of
        // the host path took 130 us longer -- the "slow DMA state" of the first 40 calls after every audit, found in round 5
        // (profiles/r5_experiments/README.md section 9).
        rc = run_passes(m, x_dev, B, T, m->audit, s, nullptr, nullptr, /*lean=*/true);
        if (rc) return rc;
        if (!m->oor_seen) {             // (possibly) no gi, no device-side fallback: was x inside fp16 range?  (if not: once more, with it)
            bool raised = false;
            if ((rc = range_flag_raised(m, s, &raised))) return rc;
            if (raised && (rc = run_passes(m, x_dev, B, T, m->audit, s, nullptr, nullptr))) return rc;
        }
        HIP_TRY(hipMemsetAsync(m->split_flag, 0, sizeof(unsigned), s));
        hipLaunchKernelGGL(k_split_audit, dim3((unsigned)std::min<size_t>((n + 255) / 256, 256 * 8)), dim3(256), 0, s,
                           (const float *)probs_dev, (const float *)m->audit, n, m->split_flag);
        HIP_TRY(hipMemcpyAsync(m->split_host, m->split_flag, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        // (a shape whose sequential scan cannot run fused -- T not a multiple of the strip -- did allocate gi: it STAYS, the
        // next audit of the shape needs it again and a hipFree of that size is 0.5 s of slow strided DMA, see above)
        float dp;
        memcpy(&dp, &m->split_host[0], sizeof(float));
        if (P.audit_passed(sp.G, m->precision, dp)) return MDK_OK;
        // the sequential result is already there
        HIP_TRY(hipMemcpyAsync(probs_dev, m->audit, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (probs_host) HIP_TRY(hipMemcpyAsync(probs_host, m->audit, n * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return MDK_OK;
    }
    if (first_attempt && pre && pre->valid && !pre->split && pre->precision == m->precision) {
        pre->valid = false;            // the sequential passes are what start_call enqueued: the caller's synchronize ends them
        m->early_used++;
        return MDK_OK;
    }
    if ((rc = forget_pre())) return rc;
    return run_passes(m, x_dev, B, T, probs_dev, s, x_host, probs_host);
}

// The first attempt of a call, enqueue only: what run_forward would launch for (x_dev, B, T) right now -- a split scan at the
// margin in use, or the sequential passes -- WITHOUT waiting for anything.  Not started (st->valid stays false; run_forward then
// does everything): timing on, a probe due, more than one pass, the exact kernels.  `prev`: the other context; where the two
// forwards cannot share the chip this one's kernels are ordered behind that one's (its result copies are not waited for).
static int start_call(mdk_gru *m, const float *x_dev, int B, int T, float *probs_dev, hipStream_t s, float *probs_host,
                      mdk_gru::Started *st, const Ctx *prev) {
    st->valid = false;
    // (GRU(256): a cluster recurrence tolerates no second forward beside it, and its time-out is read on the host)
    if (m->timing || m->variant != MDK_VARIANT_MFMA || m->wide) return MDK_OK;
    SplitPlan sp;
    int rc;
    // (the back-off of a model whose certificate was rejected at the largest margin counts calls in run_forward: a call that
    // would end it is left to run_forward)
    if (m->policy.backoff_ends_next_call()) return MDK_OK;
    const bool split = plan_split(m, B, T, sp);
    if (split && m->policy.probe_due(sp.G, m->precision)) return MDK_OK;
    const size_t budget = m->max_rows_per_pass ? m->max_rows_per_pass : kMaxRowsPerPass;
    if (!split && (size_t)B * T > budget) return MDK_OK;
    int wgs = 256;
    if (!split) {
        PassPlan P;
        HostIO io;
        io.p_host = probs_host;
        if ((rc = plan_pass(m, B, T, &io, nullptr, P))) return rc;
        wgs = P.n_wg * P.D * m->opt_gpu_share;
    }
    // two forwards side by side only where both leave the other its CUs (sequential scans of the reference's batch sizes: 100 of
    // 256 CUs each); a recurrence that holds every CU tolerates nothing beside it (profiles/r4_experiments/README.md)
    m->wait_before_l1 = nullptr;
    if (prev && prev->kernels_done && prev->last_wgs > 0 && (split || wgs + prev->last_wgs > 256)) {
        // Stage overlap (option "stage_overlap"): this batch's LAYER 0 beside the previous batch's LAYER 1 -- a layer-0 work-group
        // (8 KB of LDS, a latency chain that leaves the matrix pipe idle two thirds of its step in half precision) fits on a CU
        // beside a fused layer-1 work-group; layers of the same kind still follow each other
        static const int env_so = getenv("MDK_STAGE_OVERLAP") ? atoi(getenv("MDK_STAGE_OVERLAP")) : -1;
        const int so = env_so >= 0 ? env_so : m->opt_stage_overlap;
        const bool stage = split && m->desc.num_layers == 2 && (so == 2 || (so == 1 && m->precision == MDK_PREC_FP16));
        if (stage) {
            HIP_TRY(hipStreamWaitEvent(s, prev->l0_done, 0));
            m->wait_before_l1 = prev->kernels_done;
        } else {
            HIP_TRY(hipStreamWaitEvent(s, prev->kernels_done, 0));
        }
    }
    st->split = split;
    st->precision = m->precision;
    if (split) {
        EvTimer none{m, s};
        st->sp = sp;
        if ((rc = split_enqueue(m, sp, x_dev, probs_dev, s, nullptr, probs_host, none, &st->need_gi))) return rc;
    } else {
        if ((rc = run_passes(m, x_dev, B, T, probs_dev, s, nullptr, probs_host))) return rc;
    }
    m->wait_before_l1 = nullptr;
    st->valid = true;
    return MDK_OK;
}

// ---- the stream-ordered device forward (mdk_gru_forward_dev_async) ---------------------------------------
// run_forward waits for the certificate because the HOST decides what a split call delivers.  Here the device does: the split runs into
// probs_dev, k_split_decide reduces its certificate (and the fp32-parity probe's, half precision) into gate words, the sequential
// passes follow into probs_dev predicated on "rejected" and the audit predicated on "certified" -- each an empty launch per kernel
// when its gate is closed.  What run_forward learns from a call (margin learner, back-off, probe and audit counters, last_split) is
// learned when the call's record is retired: it is copied to a page-locked ring slot behind the call, and read once its event is done.

// one retired call: its verdict goes to the policy, as run_forward's does after its wait, with the epoch, precision and margin
// the call was enqueued with
static void retire_one(mdk_gru *m, const mdk_gru::AsyncSlot &sl, const AsyncRecord &r) {
    SplitPolicy &P = m->policy;
    P.open_record(sl.T, sl.status);
    if (!sl.split) return;
    P.record(sl.S, sl.G, sl.Tv, r.worst, r.certified);
    if (sl.probe_ran) P.probed(sl.G, r.probe_ok, r.probe_delta);
    if (sl.audited && P.audit_inflight_key == sl.audit_key) P.audit_inflight_key = 0;
    const bool current = P.is_current(sl.epoch, sl.precision, sl.G, m->precision);
    // rejected: the sequential scan was delivered.  The learner takes one step; the next call ENQUEUED after this point uses it.
    if (!r.certified) { (void)P.rejected(sl.G, current); return; }
    P.certified(sl.G, sl.precision, current);
    if (sl.audited) {
        float dp;
        memcpy(&dp, &r.audit_bits, sizeof(float));
        (void)P.audit_passed(sl.G, sl.precision, dp);      // (a failed audit: k_audit_deliver has delivered the sequential result)
    }
}

// retire the calls in flight, oldest first: those whose event is complete (`wait` = false: hipEventQuery, never blocks), or all of them
static int retire_async(mdk_gru *m, bool wait) {
    while (m->async_count) {
        const size_t i = m->async_head;
        const hipError_t e = wait ? hipEventSynchronize(m->async_slots[i].done) : hipEventQuery(m->async_slots[i].done);
        if (e == hipErrorNotReady) { (void)hipGetLastError(); break; }
        if (e != hipSuccess) return fail(MDK_ERR_DEVICE, "hipEventQuery failed: %s", hipGetErrorString(e));
        retire_one(m, m->async_slots[i], m->async_host[i]);
        m->async_head = (i + 1) % m->async_slots.size();
        m->async_count--;
    }
    return MDK_OK;
}

static void free_async(mdk_gru *m) {
    (void)retire_async(m, true);
    for (auto &sl : m->async_slots) if (sl.done) (void)hipEventDestroy(sl.done);
    m->async_slots.clear();
    m->async_head = m->async_count = 0;
    m->async_last = nullptr;
    if (m->async_host) (void)hipHostFree(m->async_host);
    m->async_host = nullptr;
    free_dev(reinterpret_cast<float *>(m->async_dev)); m->async_dev = nullptr;
    free_dev(reinterpret_cast<float *>(m->probe_flag)); m->probe_flag = nullptr;
    m->policy.probe_inflight_G = m->policy.audit_inflight_key = 0;
}

// the device words and a ring of "async_depth" slots (a new depth: every call in flight is retired first -- a wait, once)
static int ensure_async(mdk_gru *m) {
    if (!m->async_dev) {
        HIP_TRY(hipMalloc((void **)&m->async_dev, sizeof(AsyncWords)));
        HIP_TRY(hipMemset(m->async_dev, 0, sizeof(AsyncWords)));
        HIP_TRY(hipMalloc((void **)&m->probe_flag, kSplitFlagWords * sizeof(unsigned)));
    }
    const size_t depth = (size_t)m->opt_async_depth;
    if (m->async_slots.size() == depth) return MDK_OK;
    int rc;
    if ((rc = retire_async(m, true))) return rc;
    for (auto &sl : m->async_slots) if (sl.done) (void)hipEventDestroy(sl.done);
    m->async_slots.assign(depth, mdk_gru::AsyncSlot{});
    m->async_head = m->async_count = 0;
    m->async_last = nullptr;
    if (m->async_host) (void)hipHostFree(m->async_host);
    m->async_host = nullptr;
    HIP_TRY(hipHostMalloc((void **)&m->async_host, depth * sizeof(AsyncRecord), hipHostMallocDefault));
    for (auto &sl : m->async_slots) HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    return MDK_OK;
}

// one call, enqueued on `s`; the caller has dropped a batch started ahead, checked the arguments and made room in the ring
static int enqueue_async_body(mdk_gru *m, const float *x_dev, int B, int T, float *probs_dev, hipStream_t s) {
    const size_t idx = (m->async_head + m->async_count) % m->async_slots.size();
    mdk_gru::AsyncSlot &sl = m->async_slots[idx];
    sl = mdk_gru::AsyncSlot{sl.done};
    sl.T = T; sl.Tv = T; sl.precision = m->precision;
    // the workspace is the model's: this call's stream waits (on the device) for the previous call, whatever stream that was on
    if (m->async_last) HIP_TRY(hipStreamWaitEvent(s, m->async_last, 0));
    // the back-off counts calls, as in run_forward -- here calls enqueued
    SplitPolicy &P = m->policy;
    sl.status = P.begin_call();
    sl.epoch = P.learner_epoch;
    SplitPlan sp;
    int rc;
    if (!plan_split(m, B, T, sp)) {
        // not split: the sequential passes, planned with gi so that the range decision is made on the device (run_passes)
        if ((rc = run_passes(m, x_dev, B, T, probs_dev, s, nullptr, nullptr))) return rc;
    } else {
        sl.split = true; sl.S = sp.S; sl.G = sp.G; sl.Tv = sp.Tv;
        AsyncWords *w = m->async_dev;
        HIP_TRY(hipMemsetAsync(&w->gate[0], 0, sizeof(AsyncWords) - offsetof(AsyncWords, gate), s));
        EvTimer tm{m, s};
        bool need_gi = true;
        // 1. probe (half precision): the call in fp32-parity mode, its certificate into probe_flag.  Its result lands in probs_dev,
        //    which the split below overwrites in full (as in run_forward).  A probe of this margin still in flight from an earlier
        //    call is not repeated: this call is gated on that probe's verdict, which stays in the device words.
        int probe = 0;
        if (P.probe_due(sp.G, m->precision)) {
            if (!P.periodic_audit_next() && P.probe_inflight_G == sp.G) {
                probe = 2;
            } else {
                m->precision = MDK_PREC_FP32;
                rc = split_enqueue(m, sp, x_dev, probs_dev, s, nullptr, nullptr, tm, &need_gi, m->probe_flag);
                m->precision = MDK_PREC_FP16;
                if (rc) return rc;
                probe = 1;
                sl.probe_ran = true;
                P.probe_inflight_G = sp.G;
            }
        }
        // 2. the split at the margin in use, its certificate into split_flag
        if (!m->split_flag) HIP_TRY(hipMalloc((void **)&m->split_flag, kSplitFlagWords * sizeof(unsigned)));
        if ((rc = split_enqueue(m, sp, x_dev, probs_dev, s, nullptr, nullptr, tm, &need_gi, m->split_flag))) return rc;
        // 3. the decision
        hipLaunchKernelGGL(k_split_decide, dim3(1), dim3(64), 0, s, (const unsigned *)m->split_flag, (const unsigned *)m->probe_flag,
                           8 * (sp.S - 1), m->precision == MDK_PREC_FP16 ? kSplitEpsHalf : kSplitEps, probe, w);
        // 4. the repair: the sequential passes into probs_dev, empty launches unless the split was rejected.  (Bv * Tv >= B * T: the
        //    split's workspace holds them -- ensure_workspace allocates nothing after the first call at a shape.)
        if ((rc = run_passes(m, x_dev, B, T, probs_dev, s, nullptr, nullptr, false, &w->gate[0]))) return rc;
        // 5. the audit (the first call at a margin / precision, then every "scan_split_audit_every"-th split call ENQUEUED): the
        //    sequential scan into m->audit, predicated on "certified", compared in full; where it differs by more than the
        //    tolerance its result is copied over the split's by a predicated kernel
        if (const int audit_key = P.audit_due(sp.G, m->precision)) {
            const size_t n = (size_t)B * T * m->desc.num_classes;
            if ((rc = ensure_audit(m, n))) return rc;
            if ((rc = run_passes(m, x_dev, B, T, m->audit, s, nullptr, nullptr, /*lean=*/true, &w->gate[1]))) return rc;
            const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 256 * 8);
            hipLaunchKernelGGL(k_split_audit, dim3(blocks), dim3(256), 0, s, (const float *)probs_dev, (const float *)m->audit, n,
                               &w->rec.audit_bits, (const int *)&w->gate[1]);
            hipLaunchKernelGGL(k_audit_deliver, dim3(blocks), dim3(256), 0, s, probs_dev, (const float *)m->audit, n,
                               (const int *)&w->gate[1], (const unsigned *)&w->rec.audit_bits,
                               m->precision == MDK_PREC_FP16 ? kAuditTolHalf : kAuditTol);
            sl.audited = true;
            sl.audit_key = audit_key;
            P.audit_inflight_key = audit_key;
        }
        // 6. the record goes home
        HIP_TRY(hipMemcpyAsync(&m->async_host[idx], &w->rec, sizeof(AsyncRecord), hipMemcpyDeviceToHost, s));
        if ((rc = finish_timing(m, tm, s))) return rc;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sl.done, s));
    m->async_last = sl.done;
    m->async_count++;
    return MDK_OK;
}

// one call, enqueued on `s`; the caller has dropped a batch started ahead, checked the arguments and made room in the ring.  A call
// that fails part way leaves the policy as it found it: no slot will ever retire what it would have advanced (an in-flight probe
// later calls would be gated on, an audit, the cadence and back-off counters)
static int enqueue_async(mdk_gru *m, const float *x_dev, int B, int T, float *probs_dev, hipStream_t s) {
    const SplitPolicy before = m->policy;
    const int rc = enqueue_async_body(m, x_dev, B, T, probs_dev, s);
    if (rc) m->policy = before;
    return rc;
}
