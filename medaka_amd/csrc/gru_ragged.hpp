// Ragged forward (include/medaka_amd.h mdk_gru_forward_ragged / _ragged_dev): B windows of their own
// lengths in one call.  Part of api.hip (included there after gru_entries.hpp).
//
// The caller's x and probabilities are the windows one after another.  On the device the call is a rectangular batch laid out for
// its longest window: k_ragged_pad spreads x into (B, Tmax, F) with ZEROS behind every window (anything else could raise
// k_pack_x's range flag), one pass runs with PassPlan::ragged -- the recurrences hold every window's state at zero outside its own
// columns (rec_mfma.hpp RAG, exact.hpp) -- and k_ragged_unpad collects each window's own rows of the (B, Tmax, C) result.  Neither
// kernel touches the caller's buffers outside a window's rows, and padded columns are never delivered.
#pragma once

// x_pad[w][t][:] = t < len[w] ? x_cat[off[w] + t][:] : 0
static __global__ __launch_bounds__(256) void k_ragged_pad(const float *__restrict__ x_cat, float *__restrict__ x_pad,
                                                           const int *__restrict__ lens, const int *__restrict__ offs, int B, int T, int F) {
    const size_t total = (size_t)B * T * F, row = (size_t)T * F;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int w = (int)(i / row);
        const size_t r = i - (size_t)w * row;
        const int t = (int)(r / F);
        x_pad[i] = t < lens[w] ? x_cat[(size_t)offs[w] * F + r] : 0.f;
    }
}

// p_cat[off[w] + t][:] = p_pad[w][t][:] for t < len[w]
static __global__ __launch_bounds__(256) void k_ragged_unpad(const float *__restrict__ p_pad, float *__restrict__ p_cat,
                                                             const int *__restrict__ lens, const int *__restrict__ offs, int B, int T, int C) {
    const size_t total = (size_t)B * T * C, row = (size_t)T * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int w = (int)(i / row);
        const size_t r = i - (size_t)w * row;
        if ((int)(r / C) < lens[w]) p_cat[(size_t)offs[w] * C + r] = p_pad[i];
    }
}

// what both entries check before anything touches the device; *rows = sum(lengths), *Tmax = the longest window
static int ragged_args(const mdk_gru *m, const void *x, const int *lengths, int B, const void *probs, size_t *rows, int *Tmax) {
    if (!x || !probs || !lengths) return fail(MDK_ERR_ARG, "null buffer");
    if (m->wide) return fail(MDK_ERR_ARG, "ragged calls are not supported at gru_size 256 (run the windows one by one)");
    size_t n = 0;
    int tm = 0;
    for (int i = 0; i < B; ++i) {
        if (lengths[i] < 1) return fail(MDK_ERR_ARG, "window %d has length %d (every window needs at least one column)", i, lengths[i]);
        n += (size_t)lengths[i];
        tm = std::max(tm, lengths[i]);
    }
    const size_t budget = m->max_rows_per_pass ? m->max_rows_per_pass : kMaxRowsPerPass;
    const size_t area = ((size_t)B + kTileWin - 1) / kTileWin * kTileWin * (size_t)tm;
    if (area > budget)
        return fail(MDK_ERR_ARG, "the padded area of the call, %zu columns (%d windows in tiles of 8 x %d columns), exceeds the column budget "
                                 "of one pass (%zu): use fewer or shorter windows per call", area, B, tm, budget);
    *rows = n; *Tmax = tm;
    return MDK_OK;
}

// lengths (one per window slot of the largest recurrence grid: 16-window work-groups; 0 behind the batch) and offsets on the
// device, through a page-locked copy that the caller's `lengths` is consumed into before this returns.  The page-locked words
// are a ring of four: the stream-ordered copy out of a slot may still be pending when the next call comes, so a call waits on
// the host only for the copy of the call four before it (include/medaka_amd.h says so).
static int ragged_meta(mdk_gru *m, const int *lengths, int B, hipStream_t s, const int **lens_dev, const int **offs_dev) {
    const size_t n_slots = ((size_t)B + 15) / 16 * 16, need = n_slots + (size_t)B;
    mdk_gru::RagSlot &rs = m->rag_slots[m->rag_next++ % 4];
    if (rs.read) HIP_TRY(hipEventSynchronize(rs.read));
    else HIP_TRY(hipEventCreateWithFlags(&rs.read, hipEventDisableTiming));
    if (need > rs.cap) {
        if (rs.host) { (void)hipHostFree(rs.host); rs.host = nullptr; rs.cap = 0; }
        HIP_TRY(hipHostMalloc((void **)&rs.host, need * sizeof(int), hipHostMallocDefault));
        rs.cap = need;
    }
    if (need > m->rag_meta_cap) {          // (hipFree waits for the device: nothing still reads the old words)
        free_dev(m->rag_meta); m->rag_meta = nullptr; m->rag_meta_cap = 0;
        HIP_TRY(hipMalloc((void **)&m->rag_meta, need * sizeof(int)));
        m->rag_meta_cap = need;
    }
    int *h = rs.host;
    int off = 0;
    for (int i = 0; i < B; ++i) { h[i] = lengths[i]; h[n_slots + i] = off; off += lengths[i]; }
    for (size_t i = (size_t)B; i < n_slots; ++i) h[i] = 0;
    HIP_TRY(hipMemcpyAsync(m->rag_meta, h, need * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(rs.read, s));
    *lens_dev = m->rag_meta;
    *offs_dev = m->rag_meta + n_slots;
    return MDK_OK;
}

// the call on device-resident concatenated buffers, everything on `s`
static int run_ragged(mdk_gru *m, const float *x_cat, const int *lengths, int B, int Tmax, float *p_cat, hipStream_t s) {
    const int F = m->desc.num_features, C = m->desc.num_classes;
    int rc;
    memset(&m->last, 0, sizeof(m->last));
    m->last.n_layers = m->desc.num_layers;
    m->policy.open_record(Tmax, MDK_SPLIT_NOT_USED);      // always a sequential scan
    PassPlan P;
    if ((rc = plan_pass(m, B, Tmax, nullptr, nullptr, P, false, false, /*ragged=*/true))) return rc;
    const size_t padded = (size_t)B * Tmax;
    if ((rc = ensure_workspace(m, ((size_t)B + kTileWin - 1) / kTileWin * kTileWin * (size_t)Tmax, true))) return rc;
    if ((rc = ensure_staging(m, padded * F, padded * C))) return rc;
    const int *lens_dev = nullptr, *offs_dev = nullptr;
    if ((rc = ragged_meta(m, lengths, B, s, &lens_dev, &offs_dev))) return rc;
    const auto blocks = [](size_t n) { return dim3((unsigned)std::min<size_t>((n + 255) / 256, 256 * 16)); };
    hipLaunchKernelGGL(k_ragged_pad, blocks(padded * F), dim3(256), 0, s, x_cat, m->x_dev, lens_dev, offs_dev, B, Tmax, F);
    EvTimer tm{m, s};
    if ((rc = forward_pass(m, P, m->x_dev, m->p_dev, s, tm, nullptr, nullptr, nullptr, nullptr, lens_dev))) return rc;
    hipLaunchKernelGGL(k_ragged_unpad, blocks(padded * C), dim3(256), 0, s, (const float *)m->p_dev, p_cat, lens_dev, offs_dev, B, Tmax, C);
    HIP_TRY(hipGetLastError());
    if ((rc = finish_timing(m, tm, s))) return rc;
    if (m->timing && P.fuse0 && !P.exact) {      // (timing has synchronised: which twin of layer 0 ran is the range flag's word)
        int raised = 0;
        HIP_TRY(hipMemcpy(&raised, m->oor_flag, sizeof(int), hipMemcpyDeviceToHost));
        if (raised) m->last.fused_layers |= 1 << 10;
    }
    return MDK_OK;
}

extern "C" int mdk_gru_forward_ragged_dev(mdk_gru *m, const float *x_dev, const int *lengths, int B, float *probs_dev, void *stream) {
    if (!m) return fail(MDK_ERR_ARG, "null model");
    if (B < 0) return fail(MDK_ERR_ARG, "negative window count B=%d", B);
    HIP_TRY(hipSetDevice(m->device));
    drop_pending(m);                         // (first: a batch started ahead never survives an entry, whatever the entry then finds)
    if (B == 0) { memset(&m->last, 0, sizeof(m->last)); m->last.n_layers = m->desc.num_layers; return MDK_OK; }
    size_t rows = 0;
    int Tmax = 0, rc;
    if ((rc = ragged_args(m, x_dev, lengths, B, probs_dev, &rows, &Tmax))) return rc;
    // NULL = the legacy default stream, as for any HIP call
    rc = run_ragged(m, x_dev, lengths, B, Tmax, probs_dev, (hipStream_t)stream);
    if (rc) (void)hipDeviceSynchronize();    // (a half-enqueued call: nothing of it may still run when the caller sees the error)
    return rc;
}

extern "C" int mdk_gru_forward_ragged(mdk_gru *m, const float *x_host, const int *lengths, int B, float *probs_host) {
    if (!m) return fail(MDK_ERR_ARG, "null model");
    if (B < 0) return fail(MDK_ERR_ARG, "negative window count B=%d", B);
    HIP_TRY(hipSetDevice(m->device));
    drop_pending(m);
    if (B == 0) { memset(&m->last, 0, sizeof(m->last)); m->last.n_layers = m->desc.num_layers; return MDK_OK; }
    size_t rows = 0;
    int Tmax = 0, rc;
    if ((rc = ragged_args(m, x_host, lengths, B, probs_host, &rows, &Tmax))) return rc;
    const size_t nx = rows * m->desc.num_features, np = rows * m->desc.num_classes;
    if (nx > m->rag_x_cap) {
        free_dev(m->rag_x); m->rag_x = nullptr; m->rag_x_cap = 0;
        HIP_TRY(hipMalloc((void **)&m->rag_x, nx * sizeof(float)));
        m->rag_x_cap = nx;
    }
    if (np > m->rag_p_cap) {
        free_dev(m->rag_p); m->rag_p = nullptr; m->rag_p_cap = 0;
        HIP_TRY(hipMalloc((void **)&m->rag_p, np * sizeof(float)));
        m->rag_p_cap = np;
    }
    // no slab streaming: the concatenated x goes in once and the result comes out once
    hipStream_t s = m->stream;
    HIP_TRY(hipMemcpyAsync(m->rag_x, x_host, nx * sizeof(float), hipMemcpyHostToDevice, s));
    rc = run_ragged(m, m->rag_x, lengths, B, Tmax, m->rag_p, s);
    if (rc) { (void)hipDeviceSynchronize(); return rc; }   // nothing of ours may still touch the caller's buffers
    HIP_TRY(hipMemcpyAsync(probs_host, m->rag_p, np * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MDK_OK;
}
