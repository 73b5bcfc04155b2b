// q3_layers.hip — the two transformers on the device: the named GEMMs of a decoder block and of the heads, the blocks of one pass
// (q3_run_layers) and the frame step (q3_record_frame) that the engine captures into graphs, replays, or issues eagerly.
#include "q3_engine.h"

// ---- the named GEMMs of the two transformers: one descriptor builder per projection and one launch helper (q3_run_layers, q3_record_frame,
// admit_group). W8A8 (t.a8: talker_q8_0 = 2 / predictor_q8_0 = 2): xb / sc.att / sc.h hold Q8_0 blocks (int8 quants + the f32 block scales
// r.ascale / sc.asc_att / sc.asc_h) and every GEMM runs q3_launch_bgemm8: ggml's Q8_0 x Q8_0 arithmetic. Everything that
// depends on the operand format is set here, never at a call site.
// Common arguments: block l of t over the first `rows` rows of r, scratch sc; once: Q3BGemm::w_once (the Talker's 2.8 GB stream once per
// frame step; the Predictor's weights are re-read 15 times: Infinity Cache).
static Q3BGemm gemm_w(const uint4* w, const uint16_t* wscale, int K, int N, int rows, int once) {
    Q3BGemm g{}; g.w_once = once; g.B = rows; g.w = w; g.wscale = wscale; g.K = K; g.N = N;
    return g;
}
// A = the rows' norm inputs r.xb, each row scaled from its tile partials r.ssp (the fused RMSNorm)
static void a_rows(Q3BGemm& g, const Q3Tfm& t, const Q3Rows& r, float eps) {
    g.a = r.xb; g.ssp = r.ssp; g.ld_ssp = t.d / 16; g.ntiles = t.d / 16; g.d_norm = t.d; g.eps = eps;
    if (t.a8) { g.ascale = r.ascale; g.a_rt16 = r.rt16; }
}
// A = a scratch buffer of the block (sc.att / sc.h) with its block scales
static void a_scratch(Q3BGemm& g, const Q3Tfm& t, const Q3Scratch& sc, const uint16_t* a, const float* ascale) {
    g.a = a;
    if (t.a8) { g.ascale = ascale; g.a_rt16 = sc.rt16; }
}
// epilogue: += into the residual rows, and their norm inputs for the RMSNorm weight nw_next
static void y_rows(Q3BGemm& g, const Q3Tfm& t, const Q3Rows& r, const float* nw_next) {
    g.epi = Q3_EPI_RESID; g.y = r.x; g.ldy = t.d; g.yb = r.xb; g.nw_next = nw_next; g.ssp_out = r.ssp; g.ld_ssp_out = t.d / 16;
    if (t.a8) { g.yscale = r.ascale; g.y_rt16 = r.rt16; }
}
Q3BGemm q3_gemm_qkv(const Q3Tfm& t, int l, const Q3Rows& r, const Q3Scratch& sc, int rows, float eps, int once) {
    Q3BGemm g = gemm_w(t.wqkv[l], t.q8 ? t.sqkv[l] : nullptr, t.d, t.nqkv, rows, once);
    a_rows(g, t, r, eps);
    g.epi = Q3_EPI_STORE; g.y = sc.qkv; g.ldy = t.nqkv;
    return g;
}
static Q3BGemm gemm_o(const Q3Tfm& t, int l, const Q3Rows& r, const Q3Scratch& sc, int rows, int once) {
    Q3BGemm g = gemm_w(t.wo[l], t.q8 ? t.so[l] : nullptr, t.nq, t.d, rows, once);
    a_scratch(g, t, sc, sc.att, sc.asc_att);
    y_rows(g, t, r, t.ffn_norm[l]);
    return g;
}
static Q3BGemm gemm_gate_up(const Q3Tfm& t, int l, const Q3Rows& r, const Q3Scratch& sc, int rows, float eps, int once) {
    Q3BGemm g = gemm_w(t.wgu[l], t.q8 ? t.sgu[l] : nullptr, t.d, 2 * t.F, rows, once);
    a_rows(g, t, r, eps);
    g.epi = Q3_EPI_SWIGLU; g.yb = sc.h;
    if (t.a8) { g.yscale = sc.asc_h; g.y_rt16 = sc.rt16; }
    return g;
}
static Q3BGemm gemm_down(const Q3Tfm& t, int l, const Q3Rows& r, const Q3Scratch& sc, int rows, int once) {
    Q3BGemm g = gemm_w(t.wd[l], t.q8 ? t.sd[l] : nullptr, t.F, t.d, rows, once);
    a_scratch(g, t, sc, sc.h, sc.asc_h);
    y_rows(g, t, r, l + 1 < t.L ? t.attn_norm[l + 1] : t.out_norm);  // the next block's norm, or the head's
    return g;
}
// Head q = rows [q N, (q + 1) N) of output.weight (the Talker's one head: q = 0, N = its vocabulary; the Predictor's head q: N = codebook_size)
// on rows [row0, row0 + rows) of r, which hold the norm inputs for out_norm. y: the logits [rows][N] (STORE); null: the caller sets the epilogue.
Q3BGemm q3_gemm_head(const Q3Tfm& t, int q, int N, const Q3Rows& r, int row0, int rows, float eps, int once, float* y) {
    // uint4 per head (bf16 tiles of 32 k, Q8 tile pairs of 64 k) and its f16 block scales
    const size_t tile_stride = (size_t)(N / 16) * (t.d / (t.q8 ? 64 : 32)) * 64, scale_stride = (size_t)N * (t.d / 32);
    Q3BGemm g = gemm_w(t.head + tile_stride * q, t.q8 ? t.shead + scale_stride * q : nullptr, t.d, N, rows, once);
    a_rows(g, t, r, eps);
    g.a_row0 = row0; g.ssp += (size_t)row0 * (t.d / 16);
    if (y) { g.epi = Q3_EPI_STORE; g.y = y; g.ldy = N; }
    return g;
}
// Runs `launch` (returns whether it was refused) between the two events of `probe` when it is the launch e->probe_kind names.
// kind, the numbering of q3tts_k_probe: 0 gate/up, 1 QKV, 2 attention, 3 O, 4 down; -1: never probed (the heads).
template <class F>
static int probed(q3tts_engine* e, hipEvent_t* probe, int kind, hipStream_t s, F launch) {
    const bool on = probe && kind == e->probe_kind;
    if (on) hipEventRecord(probe[0], s);
    const int refused = launch() ? 1 : 0;
    if (on) hipEventRecord(probe[1], s);
    return refused;
}
// One GEMM of t in its operand format. Returns 1 when the launcher refused it (a shape it cannot run: stale activations would follow silently).
int q3_launch_gemm(q3tts_engine* e, const Q3Tfm& t, const Q3BGemm& g, hipStream_t s, hipEvent_t* probe, int kind) {
    return probed(e, probe, kind, s, [&] { return (t.a8 ? q3_launch_bgemm8(g, s) : q3_launch_bgemm(g, s)) != 0; });
}

// K1-K8 of SURVEY.md §8a: one decoder block per iteration, 5 launches — QKV GEMM (row scale from the producer's tile partials),
// attention (q/k norm + RoPE + KV append fused for decode rows), O GEMM (+ residual, + the FFN norm inputs), gate/up GEMM
// (+ SwiGLU), down GEMM (+ residual, + the next block's / the head's norm inputs). x: f32 residual rows; xb / ssp: their norm
// inputs for attn_norm[0] on entry, for out_norm on exit. Restated by oracle/q3_oracle.c tfm_layers.
// Returns the number of launches a launcher refused (a shape it cannot run: stale activations would follow silently).
int q3_run_layers(q3tts_engine* e, const Q3Tfm& t, const Q3Rows& r, const Q3LayerRun& a, Q3Scratch& sc, hipStream_t s) {
    const float eps = e->cfg.model.rms_eps;
    int bad = 0;
    const int once = &t == &e->T ? 1 : 0;
    const Q3KvCache& c = a.cache ? *a.cache : t.cache;
    for (int l = 0; l < t.L; ++l) {
        hipEvent_t* pe = l == 0 ? a.probe : nullptr;  // the probe brackets one launch of block 0
        // block 0 of a gathering pass has no QKV launch (its rows come from e->qkv0): the QKV probe then brackets block 1's, the same shape and instance
        const bool gather = a.gather && l == 0;
        if (!gather) bad += q3_launch_gemm(e, t, q3_gemm_qkv(t, l, r, sc, a.rows, eps, once), s, l == (a.gather ? 1 : 0) ? a.probe : nullptr, 1);
        Q3QkPrep qp{}; qp.qkv = sc.qkv; qp.ld = t.nqkv; qp.rows = a.rows; qp.Hq = t.Hq; qp.Hkv = t.Hkv; qp.hd = t.hd;
        qp.qnw = t.qn[l]; qp.knw = t.kn[l]; qp.eps = eps; qp.cs = t.cs; qp.sn = t.sn;
        q3_layer_cache(c, l, &qp.kc, &qp.vc, &qp.kd, &qp.vd); qp.kv8 = c.kv8 ? 1 : 0;  // (kv_q8_0: quants + scales, and the kernels of q3_attend_kv8.hip)
        qp.n_ctx = c.n_ctx; qp.row_pos = a.row_pos; qp.row_slot = a.row_slot;
        qp.slot_mod = a.slot_mod; qp.pos_const = a.pos_const;
        const bool fused = a.one_row_per_slot && t.Hq / t.Hkv >= 2;
        // the Predictor's pass A: rows [0, B) at position 0 and [B, 2B) at position 1 of an empty per-frame cache: one fused launch
        const bool pair = !a.one_row_per_slot && a.slot_mod > 0 && a.rows == 2 * a.slot_mod && a.pos_const == 0 && t.Hq / t.Hkv == 2 && t.hd == 128;
        if (!fused && !pair) bad += q3_launch_qk_prep(qp, s) ? 1 : 0;
        Q3Attend at{}; at.qkv = sc.qkv; at.ld = t.nqkv; at.rows = a.rows; at.out = (float*)sc.att; at.ldo = t.nq; at.Hq = t.Hq; at.Hkv = t.Hkv; at.hd = t.hd;
        at.kc = qp.kc; at.vc = qp.vc; at.kv8 = qp.kv8; at.kd = qp.kd; at.vd = qp.vd; at.n_ctx = c.n_ctx; at.row_pos = a.row_pos; at.row_slot = a.row_slot;
        at.fused = pair ? 2 : (fused ? 1 : 0); at.prep = qp; at.out_bf16 = 1; at.slot_mod = a.slot_mod; at.pos_const = a.pos_const;
        if (t.a8) { at.out_bf16 = 2; at.out_scale = sc.asc_att; at.out_rt16 = sc.rt16; }
        if (!fused && !pair && a.n_seg > 0) { at.seg = a.seg; at.n_seg = a.n_seg; at.seg_max_n = a.seg_max_n; at.seg_max_t = a.seg_max_t; }  // prefill of whole prompts (prefill_layers): the launch's rows as per-slot runs
        bad += probed(e, pe, 2, s, [&] { return (gather ? q3_launch_attend_gather(at, *a.gather, s) : q3_launch_attend(at, s)) != 0; });
        bad += q3_launch_gemm(e, t, gemm_o(t, l, r, sc, a.rows, once), s, pe, 3);
        bad += q3_launch_gemm(e, t, gemm_gate_up(t, l, r, sc, a.rows, eps, once), s, pe, 0);
        bad += q3_launch_gemm(e, t, gemm_down(t, l, r, sc, a.rows, once), s, pe, 4);
    }
    return bad;
}

// one frame: src/tts/engine.rs:545-642 for the slots [b0, b0 + nb) of one lane
// Returns the number of refused launches (0 = the frame was issued completely).
int q3_record_frame(q3tts_engine* e, Q3Lane& L, hipStream_t s, int B) {
    int bad = 0;
    const q3tts_model_config& m = e->cfg.model;
    const int ncb = m.n_codebooks, cbs = m.codebook_size, dp = m.p_d_model, de = m.d_embed, cap = e->cfg.max_steps_cap;
    const float eps = m.rms_eps;
    Q3Slot* slots = e->slots;
    int* codes = e->codes;
    Q3Sample sa{}; sa.logits = L.logits; sa.ld = m.t_vocab; sa.limit = m.sample_limit; sa.eos = m.eos_code; sa.slots = slots; sa.B = B; sa.row_slot = L.slot_id;
    sa.rng = e->rng; sa.codes = codes; sa.max_steps_cap = cap; sa.ncb = ncb; sa.seen = e->seen; sa.seen_words = e->seen_words;
    const bool smp = e->pred_variant != 0;  // the Predictor samples: heads store their logits, k_pred_next<true> draws from them (same launch count)
    Q3PredInput pi{}; pi.xT = L.T.x; pi.out_norm = e->T.out_norm; pi.eps = eps; pi.d = de; pi.codec0 = e->codec[0]; pi.codec0_rows = m.codec0_rows;
    pi.slots = slots; pi.row_slot = L.slot_id; pi.X = nullptr; pi.fb = L.fb; pi.B = B; pi.pproj0 = e->pproj[0]; pi.proj_b = e->proj_b; pi.dp = dp; pi.px = L.P.x;
    pi.nw = e->P.attn_norm[0]; pi.xb = L.P.xb; pi.ssp = L.P.ssp;
    if (e->P.a8) { pi.xscale = L.P.ascale; pi.x_rt16 = L.P.rt16; }  // W8A8 Predictor: every pass-A input as Q8_0 blocks
    {   // H6 (src/assets_manager.rs:383-399) for the hidden rows only (every code embedding arrives pre-projected), in the same launch
        // as the sampler: the tiles normalise the Talker's raw output rows themselves
        Q3Project pj{}; pj.x = L.T.x; pj.ldx = de; pj.rows = B; pj.w = e->proj_w; pj.bias = e->proj_b; pj.n_in = de; pj.n_out = dp; pj.y = L.P.x; pj.ldy = dp;
        pj.nw = e->P.attn_norm[0]; pj.xb = L.P.xb; pj.ssp = L.P.ssp; pj.ld_ssp = dp / 16;  // rows [0, B) of pass A
        pj.norm_w = e->T.out_norm; pj.eps = eps;
        if (e->P.a8) { pj.xscale = L.P.ascale; pj.x_rt16 = L.P.rt16; }
        bad += q3_launch_sample_input(sa, pi, pj, s) != 0;
    }
    auto pred_next = [&](int q) {
        Q3PredNext pn{}; pn.keys = L.keys; pn.n_key_parts = cbs / 16; pn.q = q; pn.ncb = ncb; pn.codec_q = e->codec[q]; pn.rows_q = m.codecq_rows; pn.d = de;
        pn.slots = slots; pn.row_slot = L.slot_id; pn.B = B; pn.codes = codes; pn.max_steps_cap = cap; pn.fb = L.fb;
        pn.tts_pad = e->tts_pad; pn.xT = L.T.x; pn.row_pos_t = L.row_pos_t; pn.pproj_q = e->pproj[q]; pn.proj_b = e->proj_b; pn.dp = dp; pn.px = L.P.x;
        const bool last = q == ncb - 1;
        pn.nw = last ? e->T.attn_norm[0] : e->P.attn_norm[0]; pn.xb = last ? L.T.xb : L.P.xb; pn.ssp = last ? L.T.ssp : L.P.ssp;
        if (last ? e->T.a8 : e->P.a8) { pn.xscale = last ? L.T.ascale : L.P.ascale; pn.x_rt16 = last ? L.T.rt16 : L.P.rt16; }  // W8A8 consumer: its first operand as Q8_0 blocks
        if (smp) { pn.plogits = L.plogits; pn.cbs = cbs; pn.prng = e->prng; pn.prng_stride = cap * (ncb - 1); }
        if (last && e->ts_variant) {  // streamed text rows instead of tts_pad; every other launch of the frame is the default's
            const Q3TextRows tr{e->text, m.text_vocab, e->ts_ids, e->ts_cnt, e->ts_cur, cap};
            bad += q3_launch_pred_last_text(pn, tr, s, smp) != 0;
        } else bad += q3_launch_pred_next(pn, s, smp) != 0;
    };
    // With the table (q3_pred_table_on), pass q >= 1 launches neither k_pred_next(q) nor block 0's QKV GEMM: block 0's attention takes the row's
    // q / k / v from qkv0[q][code_q] and its extra workgroup column records the code, adds codec_q[code_q] to fb and writes the row into P.x
    // (the O projection's residual); the row's norm inputs are not written (only the skipped GEMM read them).
    const bool tab = q3_pred_table_on(e);
    for (int q = 0; q < ncb - 1; ++q) {  // pass q produces code_{q+1}
        const int rows = q == 0 ? 2 * B : B;
        const bool gq = tab && q > 0;
        Q3AttGather gt{};
        if (gq) {
            gt.tab = q3_pred_table_slice(e, q); gt.tab_rows = q3_pred_table_rows(e); gt.keys = L.keys; gt.n_key_parts = cbs / 16; gt.q = q; gt.ncb = ncb;
            gt.codec_q = e->codec[q]; gt.d = de; gt.slots = slots; gt.row_slot = L.slot_id; gt.codes = codes; gt.max_steps_cap = cap; gt.fb = L.fb;
            gt.pproj_q = e->pproj[q]; gt.proj_b = e->proj_b; gt.dp = dp; gt.px = L.P.x;
        } else if (q > 0) pred_next(q);
        hipEvent_t* pe = nullptr;
        if (e->probe == 1 && q == 1 && B == L.nb && e->probe_i + 2 <= 8) { pe = &e->probe_ev[e->probe_i]; e->probe_i += 2; }
        // the Predictor's cache lives for one frame (src/tts/engine.rs:575: cleared per frame), so it is indexed by ROW: slot = row % B,
        // position = (q == 0 ? row / B : q + 1) — known without a load, the attention kernels request their operands at once
        bad += q3_run_layers(e, e->P, L.P, {.rows = rows, .one_row_per_slot = q > 0, .probe = pe, .slot_mod = B, .pos_const = q == 0 ? 0 : q + 1, .gather = gq ? &gt : nullptr}, L.sc, s);
        // head q on the rows that carry the newest position (pass 0: rows [B, 2B)), argmax epilogue
        Q3BGemm g = q3_gemm_head(e->P, q, cbs, L.P, q == 0 ? B : 0, B, eps, 0, smp ? L.plogits : nullptr);  // smp: the logits themselves; k_pred_next<true>(q + 1) samples from them
        if (!smp) { g.epi = Q3_EPI_ARGMAX; g.keys = L.keys; g.key_stride = cbs / 16; }  // per-tile maxima; k_pred_next(q + 1) reduces them
        bad += q3_launch_gemm(e, e->P, g, s);
    }
    pred_next(ncb - 1);
    hipEvent_t* pt = nullptr;  // probe mode 2: the Talker's layer-0 gate/up GEMM (the largest GEMM of the frame step)
    if (e->probe == 2 && B == L.nb && e->probe_i + 2 <= 8) { pt = &e->probe_ev[e->probe_i]; e->probe_i += 2; }
    bad += q3_run_layers(e, e->T, L.T, {.rows = B, .row_pos = L.row_pos_t, .row_slot = L.slot_id, .one_row_per_slot = true, .probe = pt}, L.sc, s);
    bad += q3_launch_gemm(e, e->T, q3_gemm_head(e->T, 0, m.t_vocab, L.T, 0, B, eps, 1, L.logits), s);
    return bad;
}

// one captured frame step per row bucket, of the variant e->pred_variant and e->ts_variant name
int q3_capture_frames(q3tts_engine* e, std::vector<hipGraph_t>& graphs, std::vector<hipGraphExec_t>& execs) {
    Q3Lane& L = e->lane;
    graphs.resize(e->buckets.size(), nullptr); execs.resize(e->buckets.size(), nullptr);
    for (size_t bi = 0; bi < e->buckets.size(); ++bi) {
        Q3_HIP(e, hipStreamBeginCapture(L.stream, hipStreamCaptureModeThreadLocal));
        const int refused = q3_record_frame(e, L, L.stream, e->buckets[bi]);
        Q3_HIP(e, hipStreamEndCapture(L.stream, &graphs[bi]));
        if (refused) return q3_set_err(e, Q3TTS_ERR_INVALID, "frame step: " + std::to_string(refused) + " kernel launch(es) refused for this model shape");
        Q3_HIP(e, hipGraphInstantiate(&execs[bi], graphs[bi], nullptr, nullptr, 0));
        Q3_HIP(e, hipStreamSynchronize(L.stream));
    }
    return Q3TTS_OK;
}
