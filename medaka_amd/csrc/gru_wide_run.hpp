// GRU(256) forward (gru_wide.hpp): per layer one k_gemm_rows per direction and one k_gru_wide launch for both directions, then
// k_linear_softmax.  Sequential scans only -- no split scan, no fused projection or head, no layer overlap, no early start.
// Part of api.hip (included there after gru_pass.hpp).
#pragma once

// one forward over nb windows; *timed_out = a cluster's exchange or placement handshake timed out (the result is lost)
static int wide_pass_once(mdk_gru *m, const float *x, int nb, int T, float *probs, hipStream_t s, int *timed_out) {
    const int D = m->D, L = m->desc.num_layers;
    const bool hp = m->precision == MDK_PREC_FP16;
    const WidePlan w = plan_gru_wide(nb, D, hp, m->opt_gpu_share);
    *timed_out = 0;
    if (w.work_groups > m->n_cus)
        return fail(MDK_ERR_DEVICE, "the GRU(256) cluster recurrence needs %d co-resident work-groups, the device has %d CUs",
                    w.work_groups, m->n_cus);
    const float *in = x;
    for (int l = 0; l < L; ++l) {
        const LayerDev &Ld = m->layers[l];
        float *outp = m->wact[l & 1];
        if (l == 0) {            // F <= 16 features: plain fp32, any input range (raw counts included)
            const long M = (long)nb * T;
            const unsigned blocks = (unsigned)std::min<long>((M + kG0Rows - 1) / kG0Rows, 256 * 8);
            hipLaunchKernelGGL(k_gi_wide0, dim3(blocks, (unsigned)D), dim3(192), 0, s, in, (const float *)Ld.w_ih_t,
                               (const float *)Ld.bias_gi, m->wgi, M, Ld.K);
        }
        const int KS = Ld.K / 32;
        const dim3 ggrid((unsigned)((T + kWGemmRows - 1) / kWGemmRows), (unsigned)nb);
        for (int d = 0; d < D && l > 0; ++d) {
            const half8 *wf = Ld.wih_frag + (size_t)d * 48 * KS * 2 * 64;
            const float *bias = Ld.bias_gi + (size_t)d * kGG;
            float *gi = m->wgi + (size_t)d * nb * T * kGG;
#define MDK_GGEMM(KSV, HPF)                                                                                   \
    hipLaunchKernelGGL((k_gemm_rows<KSV, HPF, 48>), ggrid, dim3(512), (size_t)2 * KSV * 4 * kWGemmBlk, s, in, wf, \
                       bias, gi, T, 0, T, Ld.wide_a_scale, Ld.wide_alpha[d])
            if (KS == 16) { if (hp) MDK_GGEMM(16, true); else MDK_GGEMM(16, false); }
            else { if (hp) MDK_GGEMM(8, true); else MDK_GGEMM(8, false); }
#undef MDK_GGEMM
        }
        // (tags restart at 1 in every launch: last launch's granules and placement headers must not look current)
        HIP_TRY(hipMemsetAsync(m->wexch, 0, (size_t)D * wide_exch_words(kGH) * sizeof(unsigned long long), s));
        const int poll = hp ? 14 : 7;            // one group per cluster: 64-clock sleeps before the first poll (as rl_lstm384)
#define MDK_GREC(NG, HPF)                                                                                            \
    hipLaunchKernelGGL((k_gru_wide<kWidePF, NG, HPF>), dim3((unsigned)w.grid, (unsigned)D), dim3(512), 0, s, (const float *)m->wgi, \
                       Ld.whh_frag, Ld.b_hn, Ld.inv_scale_rec, outp, m->wexch, m->wstatus, nb, T, D, w.n_clusters,     \
                       w.n_units, poll, 1)
        if (hp) { if (w.ngrp == 2) MDK_GREC(2, true); else MDK_GREC(1, true); }
        else { if (w.ngrp == 2) MDK_GREC(2, false); else MDK_GREC(1, false); }
#undef MDK_GREC
        m->last.rec_launches++;
        in = outp;
    }
    const long M = (long)nb * T;
    const long blocks = std::min<long>((M + 15) / 16, 256 * 8);
    if (D == 2)
        hipLaunchKernelGGL(k_linear_softmax<8>, dim3((unsigned)blocks), dim3(256), 0, s, in, m->lin_w, m->lin_b, probs, M,
                           m->desc.normalise, (const int *)nullptr);
    else
        hipLaunchKernelGGL(k_linear_softmax<4>, dim3((unsigned)blocks), dim3(256), 0, s, in, m->lin_w, m->lin_b, probs, M,
                           m->desc.normalise, (const int *)nullptr);
    HIP_TRY(hipGetLastError());
    return take_wide_status(m->wstatus, s, timed_out);
}

// A time-out is retried with growing pauses for up to "wide_wait_ms" (3 s by default), then MDK_ERR_DEVICE (retry_wide).
static int wide_pass(mdk_gru *m, const float *x, int nb, int T, float *probs, hipStream_t s) {
    return retry_wide([&](int *timed_out) { return wide_pass_once(m, x, nb, T, probs, s, timed_out); },
                      [&](int tries, long spent) {
                          return fail(MDK_ERR_DEVICE, "GRU(256) cluster exchange timed out %d times in %ld ms: the recurrence needs %d CUs of "
                                                      "the GPU at once", tries, spent,
                                      plan_gru_wide(nb, m->D, m->precision == MDK_PREC_FP16, m->opt_gpu_share).work_groups);
                      },
                      m->opt_wide_wait_ms, std::chrono::steady_clock::now());
}

// run_passes for a GRU(256) model: the same column budget per pass; x and the probabilities cross PCIe whole (host entries)
static int run_wide_passes(mdk_gru *m, const float *x_dev, int B, int T, float *probs_dev, hipStream_t s, const float *x_host,
                           float *probs_host, const int *gate) {
    if (gate) return fail(MDK_ERR_ARG, "predicated passes are not supported at gru_size 256");
    memset(&m->last, 0, sizeof(m->last));
    m->last.n_layers = m->desc.num_layers;
    // (10 KB per column and pass -- 6 KB of gi, 2 x 2 KB of activations, bidirectional -- twice H = 128's: half its column budget,
    // 84 GB at the default)
    const size_t budget = m->max_rows_per_pass ? m->max_rows_per_pass : kMaxRowsPerPass / 2;
    const size_t fit = std::max<size_t>(1, budget / (size_t)T);
    const size_t n_pass = ((size_t)B + fit - 1) / fit;
    const size_t per_pass = ((size_t)B + n_pass - 1) / n_pass;
    const size_t rows = per_pass * (size_t)T, D = m->D;
    if (rows > m->wrows) {
        free_dev(m->wgi); free_dev(m->wact[0]); free_dev(m->wact[1]);
        m->wgi = m->wact[0] = m->wact[1] = nullptr;
        m->wrows = 0;
        HIP_TRY(hipMalloc((void **)&m->wgi, D * rows * kGG * sizeof(float)));
        HIP_TRY(hipMalloc((void **)&m->wact[0], rows * D * kGH * sizeof(float)));
        if (m->desc.num_layers > 1) HIP_TRY(hipMalloc((void **)&m->wact[1], rows * D * kGH * sizeof(float)));
        m->wrows = rows;
    }
    const size_t F = m->desc.num_features, C = m->desc.num_classes;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (m->timing) {
        while (m->ev.size() < 2) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            m->ev.push_back(e);
        }
        e0 = m->ev[0]; e1 = m->ev[1];
    }
    if (x_host) HIP_TRY(hipMemcpyAsync(const_cast<float *>(x_dev), x_host, (size_t)B * T * F * sizeof(float), hipMemcpyHostToDevice, s));
    if (e0) HIP_TRY(hipEventRecord(e0, s));
    for (size_t b0 = 0; b0 < (size_t)B; b0 += per_pass) {
        const int nb = (int)std::min(per_pass, (size_t)B - b0);
        const int rec = m->last.rec_launches;
        int rc = wide_pass(m, x_dev + b0 * T * F, nb, T, probs_dev + b0 * T * C, s);
        if (rc) return rc;
        m->last.rec_launches = rec + m->desc.num_layers;       // (a re-run forward counts once)
    }
    if (e1) {
        HIP_TRY(hipEventRecord(e1, s));
        HIP_TRY(hipEventSynchronize(e1));
        HIP_TRY(hipEventElapsedTime(&m->last.total_ms, e0, e1));
    }
    HIP_TRY(hipEventRecord(m->kernels_done, s));
    m->last_wgs = 256;                                          // (nothing may share the chip with a cluster recurrence)
    if (probs_host) HIP_TRY(hipMemcpyAsync(probs_host, probs_dev, (size_t)B * T * C * sizeof(float), hipMemcpyDeviceToHost, s));
    return MDK_OK;
}
