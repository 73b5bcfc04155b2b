/*
 * q3tts.h — C ABI of the MI355X-native Qwen3-TTS inference path (libq3tts.so).
 *
 * This is the drop-in boundary for the hot path of cgisky1980/Qwen3-TTS-Rust
 * (TtsEngine::generate_with_voice -> run_inference_stream). It REPLACES the two
 * foreign runtimes the reference crate binds by hand:
 *   - the 29 dlsym'd llama.cpp symbols          (reference: src/models/llama/mod.rs:81-144,240-294)
 *   - the onnxruntime vocoder session           (reference: src/models/onnx.rs:324-459)
 * and keeps the host-visible semantics of
 *   - TtsEngine::{new,set_max_steps,set_sampler_config,generate_with_voice}
 *                                               (reference: src/tts/engine.rs:84,172,177,390)
 *   - SamplerConfig{temperature,top_k,top_p,seed}  (reference: src/tts/engine.rs:14-45)
 *   - PromptBuilder::{build_core,build_clone_prompt} (reference: src/tts/prompt.rs:141,28)
 *
 * Conventions: plain pointers and sizes, no C++ / torch types. Every function
 * returns an int status (0 = ok, <0 = error class) and leaves a message readable
 * through q3tts_last_error(). The library never aborts and never silently
 * truncates (the reference swallows vocoder-thread errors:
 * src/tts/engine.rs:496-502,520). Result buffers are allocated by the callee and
 * released with q3tts_result_free(); inputs are borrowed for the call only.
 * An engine handle is NOT re-entrant (same contract as `&mut self`,
 * src/tts/engine.rs:390); use one engine per GPU / host thread.
 */
#ifndef Q3TTS_H
#define Q3TTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Q3TTS_OK 0
#define Q3TTS_ERR_INVALID (-1)     /* bad argument / shape / config */
#define Q3TTS_ERR_DEVICE (-2)      /* HIP runtime error */
#define Q3TTS_ERR_OOM (-3)
#define Q3TTS_ERR_IO (-4)          /* weight / asset file problem */
#define Q3TTS_ERR_STATE (-5)       /* call order / handle state */
#define Q3TTS_ERR_UNSUPPORTED (-6)
#define Q3TTS_MAX_BATCH 256        /* the largest q3tts_engine_config.max_batch */

#define Q3TTS_MAX_UPSAMPLE 4
#define Q3TTS_MAX_DEC_BLOCKS 8

/* ---- model configuration (every dimension is data, never a literal) -------------------------- */

/* Autoregressive codec-token decoder: Talker + Predictor (reference: llama.cpp GGUF models loaded at
 * src/tts/engine.rs:123-137; dims read at src/models/llama/mod.rs:348-353). */
typedef struct q3tts_model_config {
    /* Talker (Qwen3 decoder: RMSNorm, QK-RMSNorm, M-RoPE, GQA, SwiGLU) */
    int32_t t_n_layer, t_d_model, t_n_head, t_n_kv_head, t_head_dim, t_d_ffn, t_vocab;
    float t_rope_theta;
    int32_t t_mrope_sections[4]; /* rotary pairs per (t,h,w,extra) section; sum == head_dim/2 */
    /* Predictor (same block, plain RoPE, 15 heads of codebook_size logits) */
    int32_t p_n_layer, p_d_model, p_n_head, p_n_kv_head, p_head_dim, p_d_ffn;
    float p_rope_theta;
    int32_t n_codebooks;   /* 16  (reference: src/tts/engine.rs:587) */
    int32_t codebook_size; /* 2048 (reference: src/tts/engine.rs:588-589) */
    float rms_eps;
    /* embedding tables (reference: src/assets_manager.rs:212-249) */
    int32_t d_embed;     /* 2048 */
    int32_t text_vocab;  /* rows of text_embd */
    int32_t codec0_rows; /* rows of codec_embd.0 (holds specials + speaker ids) */
    int32_t codecq_rows; /* rows of codec_embd.1..15 */
    /* protocol (reference: src/tts/prompt.rs:5-16, src/tts/engine.rs:555-558) */
    int32_t sample_limit; /* 2160: Talker samples over logits[0, sample_limit) */
    int32_t eos_code;     /* 2150 */
    int32_t tts_pad_id;   /* 151671: text row used as marker and tts_pad */
} q3tts_model_config;

/* Streaming neural-codec vocoder (reference: ONNX graph behind src/models/onnx.rs:342-459; state shapes
 * src/models/onnx.rs:474-495 pin latent 1024 / pre-conv 512 / 8 layers x 16 heads x 64). */
typedef struct q3tts_vocoder_config {
    int32_t n_codebooks, codebook_size, codebook_dim; /* 16, 2048, 512 */
    int32_t latent_dim;                               /* 1024 */
    int32_t pre_conv_kernel;                          /* 3 */
    int32_t n_layer, n_head, head_dim, d_ffn, sliding_window;
    float rope_theta, rms_eps, layer_scale_init;
    int32_t n_upsample;
    int32_t upsample_ratios[Q3TTS_MAX_UPSAMPLE]; /* ConvTranspose1d(k=r,s=r) + ConvNeXt each */
    int32_t decoder_dim;                         /* 1536 */
    int32_t n_dec_blocks;
    int32_t dec_rates[Q3TTS_MAX_DEC_BLOCKS]; /* 8,5,4,3 -> 1920 samples per frame with 2x2 above */
    int32_t lookahead_frames;                /* frames withheld until more input or is_last (V4) */
    int32_t sample_rate;                     /* 24000 */
} q3tts_vocoder_config;

typedef struct q3tts_engine_config {
    q3tts_model_config model;
    q3tts_vocoder_config vocoder;
    int32_t device;        /* HIP device ordinal */
    int32_t max_batch;     /* concurrent utterance slots, 1..Q3TTS_MAX_BATCH (256). Results do not depend on it. Device memory per slot:
                            *   Talker KV  2 * t_n_layer * t_n_kv_head * t_head_dim * n_ctx * 2 B  (470 MB at the 1.7B shape with n_ctx = 4096:
                            *              256 slots need a smaller n_ctx, e.g. 1024: 117 MB per slot, 30 GB); with kv_q8_0 = 1
                            *              2 * t_n_layer * t_n_kv_head * n_ctx * (t_head_dim + 2 * t_head_dim / 32) B (250 MB at n_ctx = 4096)
                            *   Predictor cache  2 * p_n_layer * p_n_kv_head * p_head_dim * 64 * 2 B
                            *   codes, Talker draws  max_steps_cap * (n_codebooks + 1) * 4 B;  Predictor draws (prng)  max_steps_cap *
                            *              (n_codebooks - 1) * 4 B;  seen codes  ceil(sample_limit / 32) * 4 B
                            *   vocoder  PCM row max_steps_cap * samples per frame * 4 B, attention rings 2 * n_layer * sliding_window *
                            *              n_head * head_dim * 4 B, the convolutions' history rows
                            * q3tts_engine_create adds these to the weights and the row buffers before it allocates anything and returns
                            * Q3TTS_ERR_OOM, with the bytes needed and the bytes free in the message, when the device has less. */
    int32_t n_ctx;         /* Talker context per slot (reference 4096: src/tts/engine.rs:133) */
    int32_t max_steps_cap; /* upper bound accepted by q3tts_set_max_steps (reference default 512) */
    int32_t with_vocoder;  /* 0: codes only (no vocoder weights allocated) */
    uint64_t synth_seed;   /* seeded synthetic weights when weights_path == NULL */
    const char* weights_path; /* NULL -> synthetic. Else the reference's quant directory (src/tts/engine.rs:91-131):
                               * qwen3_tts_talker.gguf + qwen3_tts_predictor.gguf (llama.cpp qwen3 tensor names; F32, F16,
                               * BF16, Q8_0 or the K-quants Q4_K / Q5_K / Q6_K of the gguf_q5_k_m directory, converted to
                               * bf16 at load) and qwen3_assets.gguf or its NPY fallback
                               * (src/assets_manager.rs:14-26). Shapes must match `model`: q3tts_config_from_model_dir below
                               * fills `model` and this field from the files themselves. The table row counts
                               * (text_vocab, codec0_rows, codecq_rows) are taken from the files. The vocoder
                               * (with_vocoder = 1) takes trained weights from qwen3_tts_vocoder.gguf when that file lies in this
                               * directory or, failing that, in its parent (the model directory: one unquantised file serves every
                               * quant directory); q3tts_get_vocoder_source says which it was. Without the file the vocoder's
                               * weights are the seeded synthetic ones. A file that is there but wrong (a missing tensor, a shape
                               * or metadata value that disagrees with `vocoder`, an unsupported tensor type, a value that is not
                               * finite, a file that ends early) fails q3tts_engine_create with a message naming the file and the
                               * tensor or key, before anything is allocated on the device: never a silent fall-back. Names,
                               * layouts and the precision rule: DESIGN.md section 27; tools/vocoder_to_gguf.py writes the file
                               * from a PyTorch checkpoint. */
    int32_t talker_q8_0;      /* 1: the Talker's matrices and lm_head stay ggml Q8_0 blocks ON THE DEVICE (f16 scale + 32 int8 per block,
                               * 1.06 bytes per weight instead of 2) and are multiplied in that form (W8A16: bf16 activations, every block's
                               * MFMA product scaled by f32(d)) — the reference's default quantisation (gguf_q8_0,
                               * src/tts/engine.rs:91-95). Q8_0 tensors of weights_path are kept as stored; other tensor types and the
                               * synthetic weights are quantised with ggml's reference rule. 0 (default): bf16 weights. The Predictor
                               * is not touched by this field (predictor_q8_0 below).
                               * 2: W8A8 — as 1, and every Talker GEMM's ACTIVATIONS are Q8_0 blocks too, multiplied in ggml's
                               * Q8_0 x Q8_0 arithmetic on the int8 MFMA (exact int32 block sums x f32(d_w) * d_x): what
                               * llama.cpp computes for a gguf_q8_0 directory, and what the Python API and the Rust shim select for
                               * quant = "q8_0". An activation is quantised where it is produced, from the UN-normalised v = x * nw, so
                               * its block scale carries the magnitude of the residual stream: it is d = amax / 127 rounded to f16's
                               * 11-bit significand but stored as f32 (weight scales stay f16 as in the file). Pinned by
                               * tests/test_q8_scales_{cpu,gpu}.py over rows scaled by 2^-24 .. 2^+24: bit-identical GEMM output under
                               * power-of-two scaling (eps = 0), float64 accuracy within the measured margin of ggml's order
                               * (quantise the normalised row), f16 weight scales down to 0x0001 and up to 0x7BFF. Non-finite inputs
                               * are not defined. */
    int32_t vocoder_flush_tail; /* Only matters with vocoder.lookahead_frames > 0 (V4). 0 (default): as the reference — its vocoder thread sends
                               * is_last only with a non-empty final buffer (src/tts/engine.rs:510-536), so an utterance of n_frames % 4 == 0
                               * never flushes the withheld look-ahead tail and its audio ends lookahead_frames short (restated by the oracle's
                               * q3o_chunk_plan). 1: always flush at the end of an utterance (every generated frame becomes audio). */
    int32_t predictor_q8_0;   /* 0 (default): bf16 Predictor — Q8_0 tensors of qwen3_tts_predictor.gguf are widened to bf16 at load.
                               * 2: W8A8 — the Predictor's layer matrices and its n_codebooks - 1 heads (row blocks of output.weight) stay
                               * ggml Q8_0 blocks on the device, and every Predictor GEMM, the argmax heads included, runs in the Q8_0 x Q8_0
                               * arithmetic of csrc/q3_bgemm8.hip. It shares every rule of talker_q8_0 = 2: Q8_0 tensors
                               * of the file are kept as stored, other types and the synthetic weights are quantised with ggml's reference
                               * rule; an activation is quantised where it is produced, from the un-normalised v = x * nw; block scales are
                               * amax / 127 rounded to an 11-bit significand and kept in f32. As for the Talker, parity with llama.cpp's own
                               * summation order is not pinned: the order is this library's canonical one, restated by tests/_pred_q8.py.
                               * Needs p_d_model, p_d_ffn and p_n_head * p_head_dim multiples of 512 and codebook_size a multiple of 32.
                               * 1 (W8A16 for the Predictor) is refused with Q3TTS_ERR_UNSUPPORTED; the numbering is parallel to talker_q8_0.
                               * Independent of talker_q8_0: any Talker mode combines with any Predictor mode. Opt-in: no API default
                               * selects it. */
    int32_t kv_q8_0;          /* NOTE for callers built against an earlier header: this member takes what was the struct's tail padding
                               * (sizeof is unchanged), so a struct filled member by member without q3tts_default_config or
                               * zero-initialisation hands indeterminate bytes over here — Q3TTS_ERR_INVALID, or silently a Q8_0 cache.
                               * Start every q3tts_engine_config from q3tts_default_config (or zero it) before setting members.
                               * 0 (default): the Talker's K/V cache is bf16 — no bit, launch, graph or allocation differs from an engine built
                               * before this field existed. 1: the Talker's K and V are ggml Q8_0 blocks on the device (llama.cpp's
                               * --cache-type-k q8_0 --cache-type-v q8_0): per-slot memory becomes 2 * t_n_layer * t_n_kv_head * n_ctx *
                               * (t_head_dim + 2 * t_head_dim / 32) bytes, 0.53 of bf16. Any other value: Q3TTS_ERR_INVALID. The
                               * Predictor's per-frame cache (17 keys) stays bf16. Independent of talker_q8_0 and predictor_q8_0.
                               * Blocks: 32 consecutive dims of one (position, KV head) vector — four per key, taken after q/k-norm and
                               * RoPE, four per value, taken from the raw f32 row. Quantiser: ggml's quantize_row_q8_0 in f32 (d = amax /
                               * 127, id = d ? 1 / d : 0, q = roundf(x * id), d stored as f16; a zero block has d = 0, q = 0).
                               * Arithmetic rule: the cached value is x^ = f32(d) * float(q), exact in f32, and attention is the
                               * canonical order of DESIGN.md section 4.4 unchanged with x^ wherever it has a bf16 value today — the same
                               * key-per-lane d-ascending fmaf score chain, the same 16 key-partials of the value pass, the same
                               * combination and expf. The newest key and value take part as x^ too, never as the unquantised row, so a
                               * row sees the same keys whether it was decoded or prefilled, and every kernel variant gives the same bits.
                               * The results are NOT those of the bf16 cache (ids may differ). Parity with llama.cpp's flash-attention
                               * summation order is not pinned, as for the W8A8 GEMMs. Voice prefixes are stored in the engine's format.
                               * A model shape the Q8_0-cache kernels cannot run: Q3TTS_ERR_UNSUPPORTED at q3tts_engine_create. */
} q3tts_engine_config;

typedef struct q3tts_engine q3tts_engine;
typedef struct q3tts_stream q3tts_stream;

/* Fill cfg with the Qwen3-TTS-12Hz-1.7B shape assumed by SURVEY.md §8 (28x2048 Talker, 5x1024 Predictor). */
void q3tts_default_config(q3tts_engine_config* cfg);

/* Open a model directory: every model dimension from its files (host only, no GPU). The reference gets them from llama.cpp, which reads
 * them from the two GGUFs (src/models/llama/mod.rs:348-353, src/tts/engine.rs:84-137); a caller of this library needs no knowledge of the
 * architecture either. On entry cfg holds a complete configuration (typically q3tts_default_config). On success the call overwrites
 *  - cfg->weights_path = path_buf, which receives model_dir/<quant directory> (src/tts/engine.rs:91-95: quant "q5_k_m" -> gguf_q5_k_m,
 *    "q8_0" -> gguf_q8_0, anything else including NULL -> gguf). path_buf must stay alive while cfg is used;
 *  - the fields of cfg->model the files determine. From the metadata of qwen3_tts_talker.gguf (t_*) and qwen3_tts_predictor.gguf (p_*),
 *    with A = the file's general.architecture string: A.block_count -> n_layer, A.embedding_length -> d_model, A.feed_forward_length ->
 *    d_ffn, A.attention.head_count -> n_head, A.attention.head_count_kv -> n_kv_head, A.attention.key_length -> head_dim (optional:
 *    embedding_length / head_count, llama.cpp's rule), A.rope.freq_base -> rope_theta (optional: 10000),
 *    A.attention.layer_norm_rms_epsilon -> rms_eps (one field: the two files must agree), A.rope.dimension_sections ->
 *    t_mrope_sections (Talker only, required: an integer array of 1 .. 4 entries, missing entries 0, summing to head_dim / 2).
 *    From tensor shapes: t_vocab = rows of the Talker's output.weight; n_codebooks = the number of codec_embd.N tensors of
 *    qwen3_assets.gguf (or codec_embedding_N.npy files), contiguous from 0; codebook_size = rows of the Predictor's output.weight /
 *    (n_codebooks - 1), exactly; d_embed = the codec tables' row length (= t_d_model); text_vocab (0 without a text table,
 *    src/assets_manager.rs:244-249), codec0_rows, codecq_rows = the tables' row counts (tables 1 .. must agree).
 *  - cfg->vocoder, when cfg->with_vocoder != 0 and qwen3_tts_vocoder.gguf lies in the quant directory or, failing that, in model_dir
 *    itself: every field q3tts_vocoder_config_from_file (below) takes from that file, under its checks. Without such a file, or with
 *    with_vocoder = 0, the whole vocoder block is left alone.
 * Everything else is left alone: device, max_batch, n_ctx, max_steps_cap, with_vocoder, synth_seed, talker_q8_0, predictor_q8_0, vocoder_flush_tail,
 * vocoder.layer_scale_init, and the protocol fields no file states (sample_limit, eos_code, tts_pad_id).
 * Cross-checks: proj.weight is [p_d_model][d_embed], and blk.0.attn_q / attn_k / attn_output / ffn_gate / ffn_down.weight of both files
 * have the shapes the metadata implies. What only the device path can judge, and what q3tts_engine_create checks (K % 512,
 * t_vocab % 16, ...), is not checked here: q3tts_engine_create stays the one place for that.
 * Errors go to err (err_cap bytes, always NUL-terminated when err_cap > 0; err may be NULL), not to q3tts_last_error, and leave cfg and
 * path_buf unchanged: Q3TTS_ERR_INVALID for a path_buf that is too small (the message holds the needed size), a missing or mistyped key
 * (the message names the file and the full key) and a contradiction (the key, the tensor and both numbers); Q3TTS_ERR_IO for a missing
 * or unreadable file (named). */
int q3tts_config_from_model_dir(const char* model_dir, const char* quant, q3tts_engine_config* cfg, char* path_buf, int32_t path_cap,
                                char* err, int32_t err_cap);

/* The vocoder's shape from its weights file (host only, no GPU). On entry *vc holds a complete vocoder block. On
 * success every field the file's metadata states is overwritten — with A = "q3tts-vocoder" (the file's general.architecture):
 * A.n_codebooks, A.codebook_size, A.codebook_dim, A.latent_dim, A.pre_conv_kernel, A.block_count -> n_layer, A.attention.head_count ->
 * n_head, A.attention.key_length -> head_dim, A.feed_forward_length -> d_ffn, A.attention.sliding_window, A.rope.freq_base ->
 * rope_theta, A.attention.layer_norm_rms_epsilon -> rms_eps, A.upsample_ratios (integer array; its length -> n_upsample), A.decoder_dim,
 * A.decoder_rates (integer array; its length -> n_dec_blocks), A.lookahead_frames, A.sample_rate; every key is required.
 * layer_scale_init parametrises only the synthetic generator and is left alone. Cross-checks: the numbers of codebook.N.weight tables,
 * transformer layers, up-sampling stages and decoder blocks, and the shape of every tensor the metadata implies (the tables, q_proj,
 * gate_proj, ..., the [in][out][kernel] of every ConvTranspose against its ratio, the decoder's channel halving). Errors as for
 * q3tts_config_from_model_dir: the message goes to err and names the file and the key or tensor (with both numbers), *vc stays
 * unchanged; Q3TTS_ERR_IO for a file that cannot be opened or ends early, Q3TTS_ERR_INVALID otherwise. */
int q3tts_vocoder_config_from_file(const char* path, q3tts_vocoder_config* vc, char* err, int32_t err_cap);

/* TtsEngine::new (reference: src/tts/engine.rs:84-169): allocates weights, KV slabs, vocoder state on the
 * device and builds the replayable frame-step graphs. */
int q3tts_engine_create(const q3tts_engine_config* cfg, q3tts_engine** out);
/* Where the engine's vocoder weights came from: 0 = no vocoder (with_vocoder = 0), 1 = the seeded synthetic generator, 2 = the file
 * qwen3_tts_vocoder.gguf (q3tts_engine_config.weights_path). Audio of an engine that answers 1 is the output of random filters. */
int q3tts_get_vocoder_source(const q3tts_engine* e, int32_t* source);
void q3tts_engine_destroy(q3tts_engine* e);

/* Message for the last failing call on this engine (or on this thread when e == NULL). */
const char* q3tts_last_error(const q3tts_engine* e);

/* set_sampler_config / set_max_steps (reference: src/tts/engine.rs:172-184). has_seed == 0 reproduces
 * `seed: None` (wall-clock nanoseconds, src/tts/engine.rs:473-478). */
int q3tts_set_sampler(q3tts_engine* e, float temperature, int32_t top_k, float top_p, int32_t has_seed, uint64_t seed);
int q3tts_set_max_steps(q3tts_engine* e, int32_t max_steps);

/* ---- Predictor sampler and repetition penalty ----------------------------------------------------------------------------
 * Two controls of the model family's own generation code that the reference does not have: it fixes the Predictor's sampler to greedy
 * (src/tts/engine.rs:470, LlamaSampler::greedy) and applies no penalty. Both are engine state, like the sampler above (neither
 * q3tts_request nor q3tts_engine_config grows): they apply to every request admitted after the call, which takes a snapshot of them
 * at admission. Defaults: temperature 0 (greedy) and penalty 1.0 (off) — with them every launch and every bit of the frame step is what
 * it was without these calls. The setters return Q3TTS_ERR_STATE while a session or a stream is open on the engine, and
 * Q3TTS_ERR_INVALID (state unchanged) for a NULL engine, a temperature that is negative or not finite, a top_p that is not finite, a
 * penalty that is not finite or <= 0, and a temperature > 0 on a model whose codebook_size exceeds 4096.
 * On a node the state is per engine, as the sampler's is: set it on every q3tts_node_engine(node, rank), rank 0 .. q3tts_node_size - 1,
 * before q3tts_node_generate_batch; engines left with different states make a request's result depend on the device that owns it.
 *
 * Predictor sampler: codes 1 .. n_codebooks - 1 of every frame are drawn from their head's codebook_size logits by the reference's
 * sampler (H4: src/models/llama/mod.rs:666-772 — `top_k as usize`, top-p cut inclusive, r < cumsum, the fallback), the one code 0 is
 * drawn with. temperature 0: the first maximum, no draw is consumed. The draws of a request with seed S (has_seed == 0: the wall-clock
 * seed the request resolved to) are the StdRng stream of S ^ 0x9E3779B97F4A7C15; draw frame * (n_codebooks - 1) + (q - 1) serves code q
 * of that frame, so results stay independent of batch size, slot assignment and GPU count.
 *
 * Repetition penalty p on the Talker's code-0 logits: after the min_frames EOS mask and before the sample (at temperature 0 too), every
 * logit v whose code this utterance has already GENERATED (the prompt and a voice prefix do not count) becomes v > 0 ? v / p : v * p;
 * then the chosen code is marked. force_eos_at bypasses it. p == 1.0 leaves the logits untouched. */
int q3tts_set_predictor_sampler(q3tts_engine* e, float temperature, int32_t top_k, float top_p);
int q3tts_get_predictor_sampler(const q3tts_engine* e, float* temperature, int32_t* top_k, float* top_p);
int q3tts_set_repetition_penalty(q3tts_engine* e, float penalty);   /* 1.0 = off (default) */
int q3tts_get_repetition_penalty(const q3tts_engine* e, float* penalty);

/* ---- prompt (H1: src/tts/prompt.rs:141-277 build_core, :28-118 build_clone_prompt) ------------- */
typedef struct q3tts_prompt_desc {
    const uint32_t* text_ids;     int32_t n_text;     /* tokenizer.encode(text) */
    const uint32_t* instruct_ids; int32_t n_instruct; /* NULL -> instruct == None */
    int32_t lang_id;                                  /* <0 -> None (NOTHINK control block) */
    int32_t spk_id;                                   /* <0 -> None */
    const float* spk_emb;                             /* [d_embed] or NULL */
    const int32_t* ref_codes;     int32_t n_ref_frames; /* clone path: [n_ref_frames*16] or NULL */
    const uint32_t* ref_text_ids; int32_t n_ref_text;
} q3tts_prompt_desc;

/* Builds the prompt embeddings on the device and copies them back: *out_embd = malloc'd [n_tok][d_embed] f32
 * (free with q3tts_free). */
int q3tts_build_prompt(q3tts_engine* e, const q3tts_prompt_desc* p, float** out_embd, int32_t* out_n_tok);
void q3tts_free(void* p);
/* Device-resident results for the multi-GPU gather (the one collective of the path reads device memory). With
 * enable = 1 every q3tts_generate_batch call also keeps request i's PCM in row i of an engine-owned device buffer [n][stride] f32,
 * valid until the next call on this engine; requests with want_pcm = 2 skip the host copy. q3tts_get_device_pcm returns the buffer
 * of the last call (base may be NULL before the first one). The reference has no counterpart: it is one utterance at a time on one
 * device (src/models/llama/mod.rs:413, n_seq_max = 1). */
int q3tts_set_device_pcm(q3tts_engine* e, int32_t enable);
int q3tts_get_device_pcm(q3tts_engine* e, float** base, int64_t* stride_samples, int32_t* n_rows);

/* ---- output sample rate and a one-shot resampler ---------------------------------------------------------------
 * The vocoder speaks its own rate (24 kHz). q3tts_set_output_rate(e, R) makes the engine resample on the device, by a rational
 * polyphase Kaiser-windowed sinc filter whose f32 summation order is fixed, so that everything below is reproducible bit for bit:
 *   - q3tts_generate / q3tts_generate_batch with want_pcm = 1, q3tts_stream_poll chunks (and q3tts_stream_end's PCM), session chunks in
 *     f32 and i16 carry rate R; result.sample_rate = R and result.n_samples = N(ns) = ceil(ns L / M) for ns vocoder samples, with
 *     L / M = R / 24000 in lowest terms;
 *   - a chunk that is not an utterance's last carries the outputs whose filter windows end inside the PCM produced so far,
 *     D(ns) = ceil((ns - H) L / M) minus those already delivered; the last one carries the rest. The chunks of an utterance joined are
 *     its one-shot PCM bit for bit, as at the native rate. The added latency is H input samples (104 = 4.3 ms at 8 kHz, 35 = 1.5 ms at
 *     48 kHz); first_chunk_ms keeps its meaning (the first native-rate chunk resident on the host).
 * R = 0 or the vocoder's own rate turns it off (the default): every launch and every bit is then what it is without this call.
 * Engine state like q3tts_set_predictor_sampler: Q3TTS_ERR_STATE while a session or a stream is open. Device-resident PCM
 * (q3tts_set_device_pcm, want_pcm = 2) and the node's i16 gather stay native-rate: the setter returns Q3TTS_ERR_STATE while device PCM
 * is enabled, and q3tts_set_device_pcm(e, 1) is refused while a rate is set. Q3TTS_ERR_INVALID outside 4000..96000 Hz,
 * Q3TTS_ERR_UNSUPPORTED when the pair needs more than 32768 coefficients (L x T); a refused call leaves the state as it was.
 * f32 output is not clamped (overshoot above +-1 is expected on a full-scale input); i16 is the Q3TTS_PCM_I16 rule on the resampled value.
 * The reference has neither: it emits 24 kHz and refuses clone clips at any other rate (src/tts/engine.rs:341). */
int q3tts_set_output_rate(q3tts_engine* e, int32_t rate);
int q3tts_get_output_rate(const q3tts_engine* e, int32_t* rate);   /* 0 = off */
/* One-shot: the finished clip in[0, n_in) at rate_in -> *n_out = ceil(n_in L / M) samples at rate_out in out (cap samples; too small:
 * Q3TTS_ERR_INVALID with *n_out set). Host buffers, the same kernel and table on the engine's device; the table of a pair is built once
 * and kept on the engine (64 pairs at the most). The rates must differ. This is the clone path's entry for clips that are not 24 kHz. */
int q3tts_resample(q3tts_engine* e, const float* in, int64_t n_in, int32_t rate_in, int32_t rate_out, float* out, int64_t cap, int64_t* n_out);

/* ---- speaking rate and a one-shot time-stretch -----------------------------------------------------------------
 * The model has no rate input. q3tts_set_speed(e, s) makes the engine stretch the vocoder's PCM on the device without moving its pitch,
 * by WSOLA (waveform-similarity overlap-add) whose every f32 operation and order is fixed, so that everything below is reproducible bit
 * for bit. s is the speed in per mille, 500 <= s <= 2000 (2000: twice as fast, half the samples); 0 or 1000 turns it off (the default):
 * every launch, bit, allocation, event and scheduling decision is then what it is without this call.
 * The arithmetic, at the vocoder's rate, all indices 64-bit: hop Hs = 256, window Wn = 512, offsets d in [-128, 127], HOLD = 640.
 *   x[j]: the PCM row, 0 for j < 0 and for j >= n (its valid length; nothing at or past n is ever loaded).
 *   a_k = (k Hs s) div 1000; p_{-1} = -Hs, p_0 = 0, p_k = a_k + d_k for k >= 1.
 *   d_k: with the template t[j] = x[p_{k-1} + Hs + j] (the previous frame's natural continuation) and c(d) = sum_{j < Wn} x[a_k + d + j] t[j]
 *     — one sequential f32 chain in ascending j, acc = acc + x * t with one rounded multiply and one rounded add per step, never
 *     contracted — d_k is the FIRST maximum of c in ascending d. Non-finite PCM is not defined.
 *   w[j] = 0.5 - 0.5 cos(2 pi j / Wn), computed in double and rounded once to f32.
 *   y[m], k = m div Hs, j = m mod Hs: (w[j + Hs] * x[p_{k-1} + j + Hs]) + (w[j] * x[p_k + j]), two rounded multiplies and one rounded add.
 *   A finished row of n samples gives N_t(n) = ceil(n 1000 / s) outputs, every frame k < ceil(N_t / Hs) decided with zeros behind n.
 *   On an unfinished row frame k is decidable iff need_k + HOLD <= n, need_0 = 0, need_k = max(a_k, a_{k-1} + Hs): the rule knows no d, and
 *   a decidable frame never reads at or beyond n. D_t(n) = Hs x (the number of leading decidable frames).
 * What follows the speed:
 *   - q3tts_generate / q3tts_generate_batch with want_pcm = 1, q3tts_stream_poll chunks (and q3tts_stream_end's PCM), session chunks in f32
 *     and i16; result.n_samples = N_t(ns) for ns vocoder samples. sample_rate is untouched, first_chunk_ms keeps its meaning (the first
 *     unstretched chunk resident on the host). The codes, n_frames and hit_eos are those of the unstretched run.
 *   - a chunk that is not an utterance's last carries D_t(ns) minus what was delivered; the last one the rest. The chunks of an utterance
 *     joined are its one-shot PCM bit for bit, whatever the batch, the slot, the schedule or the swap history. The added latency is HOLD
 *     input samples (26.7 ms) plus at most one hop.
 *   - with an output rate set as well, the resampler reads the stretched row (valid length N_t or D_t, the same finished flag):
 *     the result is q3tts_resample(q3tts_time_stretch(native PCM)).
 * Engine state like q3tts_set_output_rate: Q3TTS_ERR_STATE while a session or a stream is open and while q3tts_set_device_pcm is enabled
 * (device-resident PCM, want_pcm = 2 and the node's gather stay unstretched; q3tts_set_device_pcm(e, 1) is refused while a speed is set);
 * Q3TTS_ERR_INVALID outside 500..2000 and on an engine without a vocoder; Q3TTS_ERR_OOM, naming the bytes needed and the bytes free, when
 * the stretched rows do not fit the device. A refused call leaves the state as it was. The speed is the engine's, not a request's.
 * The constants are quality parameters that nobody has listened to yet. The reference has no counterpart. */
int q3tts_set_speed(q3tts_engine* e, int32_t permille);
int q3tts_get_speed(const q3tts_engine* e, int32_t* permille);   /* 0 = off */
/* One-shot: the finished clip in[0, n_in) -> *n_out = ceil(n_in 1000 / permille) samples in out (cap samples; too small:
 * Q3TTS_ERR_INVALID with *n_out set). Host buffers, the same kernel on the engine's device; permille in 500..2000 and not 1000. */
int q3tts_time_stretch(q3tts_engine* e, const float* in, int64_t n_in, int32_t permille, float* out, int64_t cap, int64_t* n_out);

/* ---- generation (run_inference_stream: src/tts/engine.rs:445-656) ------------------------------ */
typedef struct q3tts_prefix q3tts_prefix;  /* a voice prefix: see "voice prefixes" below */
typedef struct q3tts_request {
    const float* prompt_embd; int32_t n_tok; /* [n_tok][d_embed] f32 host rows (PromptData.embd), or NULL ... */
    int32_t text_stream;  /* 1: the streamed text layout (see "streaming text input"): only the first text id is in the prompt, the rest
                           * joins the feedback rows. Needs `prompt` with n_text >= 1. Any other value: the whole text is in the prompt
                           * (the reference). This field and text_open occupy the two 4-byte alignment gaps the struct always had (behind
                           * n_tok and behind has_seed): no field moved, sizeof is 80 as before, `prefix` is still the last field, and a
                           * caller that zero-fills its requests gets the behaviour it had */
    const q3tts_prompt_desc* prompt;         /* ... to build from ids on the device */
    int32_t use_engine_sampler;              /* 1: ignore the five fields below, use q3tts_set_sampler state */
    float temperature; int32_t top_k; float top_p; int32_t has_seed;
    int32_t text_open;    /* sessions only, with text_stream = 1: 1 = more text follows through q3tts_session_append_text; else the text is closed */
    uint64_t seed;
    int32_t max_steps;    /* 0 -> engine value */
    int32_t min_frames;   /* bench control: EOS logit masked while n_frames < min_frames (0 = reference) */
    int32_t force_eos_at; /* bench control: EOS forced at this step (<0 = off) */
    int32_t want_pcm;     /* 0: codec ids only; 1: PCM in host memory; 2: PCM kept on the device only (q3tts_set_device_pcm) */
    const q3tts_prefix* prefix; /* NULL: the prompt is prompt_embd / prompt alone. Else the prompt is the prefix's rows followed by this
                                 * request's own rows: prompt_embd / n_tok, or `prompt` as a text-only desc (see "voice prefixes") */
} q3tts_request;

typedef struct q3tts_result {
    int32_t status;
    int32_t n_frames;      /* frames kept (EOS frame excluded, as src/tts/engine.rs:558-562) */
    int32_t hit_eos;
    int32_t* codes;        /* [n_frames][n_codebooks] raw ids (unclamped) */
    float* pcm;            /* [n_samples] mono f32, or NULL; pinned host memory: release with q3tts_result_free only */
    int32_t n_samples;
    int32_t sample_rate;
    float first_chunk_ms;  /* entry -> first 4-frame PCM chunk resident on host (0 if none) */
    float total_ms;
} q3tts_result;

int q3tts_generate(q3tts_engine* e, const q3tts_request* req, q3tts_result* out);
/* Continuous batching over max_batch slots; results are independent of n, of slot assignment and of the
 * number of GPUs the caller shards over (per-utterance RNG stream is a function of req->seed only). */
int q3tts_generate_batch(q3tts_engine* e, const q3tts_request* reqs, int32_t n, q3tts_result* outs);
void q3tts_result_free(q3tts_result* r);

/* Streaming: 4-frame (64-code) chunks as in the reference's vocoder thread (src/tts/engine.rs:507-541). */
int q3tts_stream_begin(q3tts_engine* e, const q3tts_request* req, q3tts_stream** out);
/* Blocks until the next chunk; *chunk is owned by the stream and valid until the next poll/end. */
int q3tts_stream_poll(q3tts_stream* s, const float** chunk, int32_t* n_samples, int32_t* is_final);
int q3tts_stream_end(q3tts_stream* s, q3tts_result* out_codes_optional);

/* ---- voice prefixes: prefill a voice prompt once, reuse its Talker K/V ----------------------------------------------------
 * A prompt is a voice part (the optional instruct block, the role block, the control block, the speaker row and, for a cloned voice,
 * BOS ref_text EOS, the codec-BOS row, one row per reference frame and a PAD row) followed by a text part of n_text + 3 rows (BOS, the
 * text, EOS, the activation row). Requests in the same voice, language and instruct share the voice part. A prefix holds the Talker's
 * K/V of such a part on the device; a request that names it starts from a copy of them instead of running those rows again. The
 * reference has no counterpart (it serves one request at a time and rebuilds the whole prompt each call, src/tts/engine.rs:390-466).
 *
 * q3tts_prefix_create: exactly one of p (its voice fields; n_text must be 0) or embd / n_tok (host rows [n_tok][d_embed]) is given;
 * 1 <= rows < n_ctx. Refused (Q3TTS_ERR_STATE) while a session is open — the session makes prefixes itself then ("voices in a session"
 * below: q3tts_session_prefix_create, q3tts_session_submit_keep_voice). Destroy every prefix before its engine.
 * A request with prefix != NULL:
 *  - its prompt_embd / n_tok are the rows after the prefix; otherwise `prompt` builds only the text part: text_ids are used and every
 *    voice field must be in its None state (instruct_ids NULL, lang_id < 0, spk_id < 0, spk_emb NULL, ref_codes NULL, ref_text_ids NULL),
 *    else Q3TTS_ERR_INVALID with a message naming the field;
 *  - it needs P + n + max_steps <= n_ctx (P prefix rows, n own rows), else it fails by itself as any request does;
 *  - a prefix made by another engine is Q3TTS_ERR_INVALID; q3tts_node_generate_batch refuses requests with a prefix (Q3TTS_ERR_INVALID).
 * Contract: with a prefix made from voice desc V and a request with text T, the results (codes, hit_eos, PCM, streamed chunks) are
 * bit-identical to those of the same request without a prefix whose desc is V with text T — in every talker_q8_0 mode, through
 * q3tts_generate, q3tts_generate_batch, q3tts_stream_* and sessions. (Every row's arithmetic depends only on that row and the K/V at its own
 * and earlier positions, in an order that does not depend on the batch: DESIGN.md §4.) A session keeps the pointer, not a copy: the prefix
 * outlives it because q3tts_prefix_destroy is refused while a session is open. */
int q3tts_prefix_create(q3tts_engine* e, const q3tts_prompt_desc* p, const float* embd, int32_t n_tok, q3tts_prefix** out);
int32_t q3tts_prefix_rows(const q3tts_prefix* x);
int q3tts_prefix_destroy(q3tts_prefix* x);   /* Q3TTS_ERR_STATE while a session is open on its engine */

/* ---- sessions: continuous batching with per-request streaming ------------------------------------------------------------
 * The serving form of run_inference_stream (src/tts/engine.rs:445-656) for many utterances at once: requests are submitted into a
 * running batch at any time, each request's 4-frame chunks are delivered as they are produced, and a request can be cancelled.
 * One worker thread per session drives the engine's max_batch slots: between 4-frame chunks it admits queued requests into free
 * slots, retires cancelled ones, runs the frame steps and the batched vocoder, and gathers every slot's new PCM with one kernel launch
 * and one device-to-host copy into pinned staging.
 *
 * Ownership: an open session owns its engine. While it is open, q3tts_generate / q3tts_generate_batch, q3tts_stream_begin, every
 * q3tts_k_* call that takes the engine, q3tts_set_sampler / q3tts_set_max_steps / q3tts_set_device_pcm, q3tts_build_prompt, q3tts_mel,
 * the q3tts_clone_* calls and a second q3tts_session_create return Q3TTS_ERR_STATE. After q3tts_session_close the engine is usable as
 * before. The engine needs with_vocoder = 1.
 *
 * Contract:
 *  - Per id, events come in order. Every accepted id gets exactly one final event: DONE, FAILED or CANCELLED (is_final = 1). The
 *    last CHUNK of a DONE request has is_final = 1 (it may carry 0 samples when the utterance ends on a chunk boundary).
 *  - A request's chunks have the sample counts q3tts_stream_poll gives for the same request (4-frame chunks, the V4 look-ahead rule
 *    of the reference's vocoder thread, vocoder_flush_tail honoured; empty polls produce no CHUNK). Joined, they are bit-identical to
 *    the PCM q3tts_generate_batch returns for that request: results do not depend on slot, batch size or admission time.
 *  - A request that fails by itself (e.g. prompt + max_steps > n_ctx) gets a FAILED event with its status; other requests are
 *    unaffected. A device error in the worker fails every open request with Q3TTS_ERR_DEVICE (other internal errors with their
 *    status); the session then refuses new submissions. Nothing is retried.
 *  - Memory is bounded: PCM goes through Q3TTS_SESSION_RING_DEPTH pinned staging buffers of max_batch x (4 + lookahead_frames) x
 *    samples per frame samples each (f32: 4 bytes, i16: 2), plus one device buffer of that size. When every staging buffer still
 *    holds chunks the consumer has not taken, the worker waits (decoding pauses) instead of allocating.
 */
typedef struct q3tts_session q3tts_session;
#define Q3TTS_SESSION_RING_DEPTH 4
#define Q3TTS_PCM_F32 0
#define Q3TTS_PCM_I16 1   /* (x * 32767).clamp(-32768, 32767) as i16, truncation toward zero (src/utils/audio.rs:35-37) */
#define Q3TTS_EV_NONE 0
#define Q3TTS_EV_CHUNK 1
#define Q3TTS_EV_DONE 2
#define Q3TTS_EV_FAILED 3
#define Q3TTS_EV_CANCELLED 4
typedef struct q3tts_session_event {
    uint64_t id;
    int32_t kind;          /* Q3TTS_EV_* */
    int32_t status;        /* FAILED: the request's error status; else Q3TTS_OK */
    const void* pcm;       /* CHUNK: n_samples f32 or i16 samples (the session's format), owned by the session and valid until the next
                            * q3tts_session_next call; NULL otherwise */
    int32_t n_samples;
    int32_t is_final;      /* 1 on the last CHUNK of a request and on every final event */
    q3tts_result result;   /* final events: status, codes, n_frames, hit_eos, n_samples (delivered in chunks), sample_rate,
                            * first_chunk_ms (submit -> first chunk ready for the consumer), total_ms (submit -> final event ready).
                            * pcm is always NULL (the audio went out as chunks). The caller releases it with q3tts_result_free. */
} q3tts_session_event;
/* pcm_format: Q3TTS_PCM_F32 or Q3TTS_PCM_I16. Starts the worker thread. */
int q3tts_session_create(q3tts_engine* e, int32_t pcm_format, q3tts_session** out);
/* Thread-safe, any time. The request and everything it points to are copied before the call returns. req->want_pcm is ignored: a
 * session always produces PCM, in its own format. *id receives the request's id (ids start at 1). Q3TTS_ERR_STATE after a worker
 * failure. Requests are validated (prompt size, max_steps) at admission: failures arrive as FAILED events. */
int q3tts_session_submit(q3tts_session* s, const q3tts_request* req, uint64_t* id);
/* Thread-safe. Takes effect at the next chunk boundary; from the moment it returns no further CHUNK of the id is delivered, and its
 * final event is CANCELLED. Q3TTS_ERR_INVALID for an unknown id or one whose final event was already delivered. */
int q3tts_session_cancel(q3tts_session* s, uint64_t id);
/* One consumer thread. Blocks until an event is ready or timeout_ms runs out (< 0: no limit); a timeout returns Q3TTS_OK with
 * ev->kind = Q3TTS_EV_NONE. */
int q3tts_session_next(q3tts_session* s, int32_t timeout_ms, q3tts_session_event* ev);
/* Cancels everything queued or running, stops the worker and frees the session (events not consumed are discarded and their results
 * freed). Must not run concurrently with q3tts_session_next. Returns the worker's error status, if it failed. */
int q3tts_session_close(q3tts_session* s);
/* Message of the last failing session call or of the worker's failure. */
const char* q3tts_session_last_error(const q3tts_session* s);

/* ---- voices in a session: create prefixes and clone voices while the batch runs --------------------------------
 * Voice work as part of the running batch. Prefix jobs and requests share the session's one FIFO; the worker stays the only thread that
 * touches the GPU. The reference has no counterpart.
 *
 *  - q3tts_session_prefix_create: a standalone prefix job, arguments as q3tts_prefix_create (copied before it returns). At a chunk
 *    boundary its voice rows take a free slot, ride the same batched prefill as the requests admitted there, and the slot's first P
 *    positions are copied into the prefix's store; the slot is free again from the next boundary. 1 <= P < n_ctx.
 *  - q3tts_session_submit_keep_voice: a whole-prompt request whose voice part is kept. After its prefill the first voice_rows positions
 *    of its slot are copied into the store: no second prefill. voice_rows = 0 takes the voice part of req->prompt (the whole prompt
 *    minus its n_text + 3 text rows, 2 with text_stream); a prompt_embd request states it (1 <= voice_rows < n_tok). A request that
 *    names a prefix cannot keep one (Q3TTS_ERR_INVALID).
 *    Either store is byte for byte the one q3tts_prefix_create makes of the same rows.
 *  - Both are thread-safe, return at once and hand out a handle that is valid immediately, in the pending state: q3tts_prefix_state is 0
 *    (pending), 1 (ready) or < 0 (the status it failed with); q3tts_prefix_rows is 0 until it is ready. When the store is written (or the
 *    entry failed) a Q3TTS_EV_PREFIX event with the call's id and the status is published: is_final = 1 for a job, 0 for a keep-voice
 *    request, whose own events follow as usual. A keep-voice request that fails at admission fails its prefix with the same status; one
 *    cancelled before admission (and a cancelled job) fails it with Q3TTS_ERR_STATE, and the PREFIX event says so.
 *  - A request may name a pending prefix: the worker does not take it, or anything behind it in the FIFO, until the prefix is ready. If
 *    the prefix failed, the request gets FAILED / Q3TTS_ERR_INVALID with a message. Prefixes made before the session opened work as ever.
 *  - q3tts_session_prefix_release (thread-safe) gives a handle back during the session, whatever its state: a later submit that names it
 *    returns Q3TTS_ERR_INVALID, and the worker frees the store once no queued request names it (admitted requests hold their own copy).
 *    Every handle is given back exactly once: released during the session, or passed to q3tts_prefix_destroy after
 *    q3tts_session_close. Close cancels pending jobs, whose handles then read failed; ready prefixes survive it as ordinary prefixes.
 *  - q3tts_session_clone blocks its caller while the worker runs the clone encoders between two chunk boundaries, on the engine's
 *    stream: audio at `rate` Hz (converted to 24000 Hz by the device resampler first when it differs, as q3tts_resample does) -> codes
 *    [n_frames][ae_n_codebooks] and the speaker embedding, bit for bit what q3tts_clone_audio_encode / q3tts_clone_speaker_encode give
 *    outside a session. Either output may be NULL. Q3TTS_ERR_STATE before q3tts_clone_init ("not loaded"), and once the session is
 *    closing or its worker has failed (a waiting caller is woken then). Clone calls do not queue behind requests, and the caller may
 *    be the consumer thread: a worker that waits for staging space (events nobody reads meanwhile) serves clone calls while it waits.
 * Still refused while a session is open (Q3TTS_ERR_STATE): q3tts_prefix_create, q3tts_prefix_destroy, q3tts_clone_audio_encode,
 * q3tts_clone_speaker_encode, q3tts_clone_init, q3tts_mel, q3tts_resample, and everything "sessions" lists above. */
#define Q3TTS_EV_PREFIX 5
int q3tts_session_prefix_create(q3tts_session* s, const q3tts_prompt_desc* p, const float* embd, int32_t n_tok,
                                q3tts_prefix** out, uint64_t* id);
int q3tts_session_submit_keep_voice(q3tts_session* s, const q3tts_request* req, int32_t voice_rows /* 0: from the desc */,
                                    uint64_t* id, q3tts_prefix** out);
int q3tts_session_prefix_release(q3tts_session* s, q3tts_prefix* x);
int q3tts_session_clone(q3tts_session* s, const float* audio, int64_t n_samples, int32_t rate,
                        int64_t* codes, int32_t cap_frames, int32_t* n_frames, float* spk_emb);
int32_t q3tts_prefix_state(const q3tts_prefix* x);   /* 0 pending, 1 ready, < 0 the status it failed with */

/* ---- streaming text input: feed a running request its text as it arrives ---------------------------------------
 * The reference puts a request's whole text into the prompt (build_core, src/tts/prompt.rs:229-264) and adds tts_pad to every feedback
 * row (src/tts/engine.rs:622-631). request.text_stream = 1 selects the model's second layout, in which a sentence can start to sound
 * after its first word. PARITY IS UNPINNED: the reference crate has only the whole-text layout and no other implementation was at hand,
 * so the contract is the layout as written here (tests/_text_stream.py restates it on the CPU):
 *   - the voice part of the prompt (instruct, role and control blocks, speaker row, clone rows) is unchanged, so voice prefixes compose
 *     with streaming (a text-only desc behind request.prefix);
 *   - with text ids x[0, n), n >= 1, the text part is two rows instead of n + 3: text[tts_bos] + codec0[PAD], then
 *     text[x[0]] + codec0[BOS] (in place of the activation row text[tts_pad] + codec0[BOS]);
 *   - the trailing rows are T[j] = text[x[j + 1]] for j < n - 1, and T[n - 1] = text[tts_eos] once the text is closed;
 *   - after frame f the Talker's next input row is fb + T[f] when f < len(T), else fb + tts_pad, in f32 as (fb + codec_15) + row.
 * Table look-ups follow the prompt builder's out-of-range rule. prompt_embd with text_stream = 1, and n_text = 0, are Q3TTS_ERR_INVALID.
 * q3tts_generate, q3tts_generate_batch and q3tts_stream_begin take closed text and never wait: text_open = 1 is Q3TTS_ERR_INVALID there.
 * q3tts_node_generate_batch refuses text_stream (Q3TTS_ERR_INVALID). Streamed and whole-text requests mix freely in a batch; a request
 * with text_stream = 0 computes exactly what it did before.
 *
 * In a session a request submitted with text_open = 1 receives more text while it runs:
 *   q3tts_session_append_text(s, id, ids, n, close) appends ids[0, n) (copied) and, with close = 1, ends the text; n = 0 with close = 1
 *   only ends it. Thread-safe. Q3TTS_ERR_INVALID for a NULL session, NULL ids with n > 0, n < 0, an unknown or finished id, a request
 *   without text_stream and text that is already closed. Trailing rows beyond the request's max_steps are accepted and never read.
 * Readiness: a request at n_frames = f takes part in the next chunk of 4 frame steps iff its text is closed or len(T) >= f + 4 (those
 * steps read T[f .. f + 3]); otherwise it is PARKED for that chunk boundary: it produces nothing and loses nothing, and what it produces
 * is bit for bit what the same text gives when it is all there at submission. A request that stays open and is never fed stays parked
 * (the worker sleeps; an append wakes it); q3tts_session_cancel and q3tts_session_close end it. The reference has no counterpart. */
int q3tts_session_append_text(q3tts_session* s, uint64_t id, const uint32_t* ids, int32_t n, int32_t close);

/* ---- paced requests and swapping: a listener says how far ahead its request may run; a parked request leaves its slot ----
 * A session synthesises many times faster than a listener plays, and a request holds its slot until its final event. Two calls let a
 * GPU serve more open requests than it has slots: a frame CREDIT per request (pacing), and moving a parked request's whole state into
 * a device arena and later into any free slot (swapping). Neither is on unless asked for: with q3tts_session_set_swap never called and
 * no paced submission, no launch, bit, event or scheduling decision differs.
 *
 * CONTRACT. For any schedule of grants, text arrivals, swap-outs and swap-ins, a request's events are those of the same request through
 * q3tts_session_submit: the same chunk sample counts in the same order; the chunks joined equal q3tts_generate_batch's PCM bit for bit
 * (f32 and i16, with and without an output rate); the same codes, n_frames and hit_eos — in every talker_q8_0 / predictor_q8_0 /
 * kv_q8_0 mode, with voice prefixes, the Predictor sampler and the repetition penalty. Other requests' results do not change.
 *
 *   q3tts_session_submit_paced(s, req, credit_frames, &id): q3tts_session_submit plus a frame credit. credit_frames >= 4, else
 *     Q3TTS_ERR_INVALID. There is no paced form of q3tts_session_submit_keep_voice: a keep-voice request runs unpaced.
 *   q3tts_session_grant(s, id, frames): thread-safe, at any time. frames > 0 adds to the credit; frames < 0 lifts the limit for good.
 *     Q3TTS_ERR_INVALID for frames == 0, an unknown or finished id, and an id that was not submitted paced.
 *   The credit rule: at a chunk boundary a paced request with n frames so far takes the next chunk iff n + 4 <= credit. Otherwise it is
 *     parked exactly as a text-starved request is ("streaming text input"); a request that is both paced and text_stream runs when both
 *     rules allow it. A grant wakes the worker as an append does.
 *   q3tts_session_set_swap(s, arena_bytes): valid before the first submission (Q3TTS_ERR_STATE later). 0 (the default): off. Otherwise
 *     one device arena of that size for the session's lifetime, checked against the device's free memory as q3tts_engine_create checks its
 *     own sum (Q3TTS_ERR_OOM, the message names both numbers), freed by q3tts_session_close. The arena is carved on the host — first fit
 *     over 256-byte units, neighbours coalesced on free — so no chunk boundary allocates or frees device memory.
 *   With swapping on, while the slots wanted (swapped-out requests whose rule holds again, and the queue's admissible head) exceed the
 *     free ones, parked slots are swapped out, longest-parked first; a running request is never preempted; with no room in the arena the
 *     slot stays parked and nothing fails. Swapped-out requests whose rule holds again take free slots oldest-ready first, ahead of new
 *     admissions. A slot freed by a swap-out is refilled at the NEXT boundary. q3tts_session_cancel, q3tts_session_close and a worker
 *     failure treat a swapped-out request as any open one (exactly one final event; its block is freed); q3tts_session_append_text keeps
 *     working (the text is uploaded whole at swap-in).
 *   q3tts_session_swap_stats(s, out): out[0] swap-outs, [1] swap-ins, [2] swap-ins into a slot other than the one left, [3] arena bytes
 *     in use, [4] their peak, [5] swap-outs skipped because the arena had no room. A block counts as in use until the last copy that
 *     read or wrote it has run on the device: its bytes are not handed out again before that.
 * Every call refuses a NULL session with Q3TTS_ERR_INVALID ("null session").
 *
 * MEMORY. Beside the per-slot memory stated at q3tts_engine_config.kv_q8_0 (the Talker's K/V: n_ctx positions per slot), a swapped-out request at Talker
 * position cur_pos whose vocoder has taken f frames occupies one block of
 *     2 * store(np) + S + up16(f * samples_per_frame * 4)      bytes, rounded up to 256,
 * np = ceil(cur_pos / 64) * 64; store(np) = t_n_layer * t_n_kv_head * np * t_head_dim * 2 (kv_q8_0: * 17 / 16 instead of * 2), one
 * voice-prefix store each for K and V; S = the sum, each term rounded up to 16, of max_steps_cap * 4 * (n_codebooks + 1 + n_codebooks - 1)
 * (codes, both samplers' draws), ceil(sample_limit / 32) * 4 (codes 0 seen), 4 * (t_vocab + t_d_model) (the parked rows), the vocoder's
 * per-slot history blocks (what a slot's reset zeroes) and 2 * n_layer * (sliding_window + 4) * n_head * head_dim * 4 (its rings); the
 * last term is the produced part of the slot's PCM row. */
int q3tts_session_submit_paced(q3tts_session* s, const q3tts_request* req, int32_t credit_frames, uint64_t* id);
int q3tts_session_grant(q3tts_session* s, uint64_t id, int32_t frames);
int q3tts_session_set_swap(q3tts_session* s, int64_t arena_bytes);
int q3tts_session_swap_stats(const q3tts_session* s, int64_t out[6]);

/* ---- one node, several GPUs ----------------------------------------------------------------------
 * The reference is one utterance at a time on one device (n_seq_max = 1, src/models/llama/mod.rs:413; `&mut self`,
 * src/tts/engine.rs:390). Utterances share nothing but read-only weights, so a batch shards over independent units:
 * q3tts_node_create builds one engine (full weight replica) and one host thread per listed device; request i of a
 * q3tts_node_generate_batch call runs on device i mod n_devices (order preserved, results independent of n_devices: the
 * sampler stream is a function of req->seed only). There is no data-path collective. With pcm_i16 != NULL the finished
 * PCM stays on the devices, is converted there to 16-bit samples exactly as the reference saves audio
 * (src/utils/audio.rs:35-37: (x * 32767).clamp(-32768, 32767) as i16) and gathered to the FIRST listed device with RCCL
 * over xGMI — one ncclAllGather of the per-utterance sample counts, one group of ncclSend / ncclRecv — then copied to the
 * host once: pcm_i16[i] = malloc'd [outs[i].n_samples] samples of request i (release with q3tts_free; outs[i].pcm stays
 * NULL). With pcm_i16 == NULL requests behave as in q3tts_generate_batch (want_pcm = 1: f32 PCM in host memory) and RCCL
 * is never loaded. RCCL is resolved at run time (librccl.so.1); a node handle is not re-entrant.
 * Errors: a request that fails by itself (e.g. prompt + max_steps > n_ctx) carries its own outs[i].status and the call still returns
 * Q3TTS_OK with every other result intact. When a device or the gather fails the call returns the error, every outs[i] — including
 * the results of the devices that succeeded — is still valid to pass to q3tts_result_free, and no pcm_i16[i] is left allocated. */
typedef struct q3tts_node q3tts_node;
typedef struct q3tts_node_timings {
    float generate_ms;      /* slowest device: its q3tts_generate_batch wall time */
    float gather_ms;        /* pack + collectives + copy to the host (0 without pcm_i16) */
    float total_ms;
    int64_t gathered_bytes; /* i16 PCM bytes that reached the host through device 0 */
    int32_t n_devices;
} q3tts_node_timings;
int q3tts_node_create(const q3tts_engine_config* cfg /* .device is ignored */, const int32_t* devices, int32_t n_devices, q3tts_node** out);
void q3tts_node_destroy(q3tts_node* n);
int q3tts_node_generate_batch(q3tts_node* n, const q3tts_request* reqs, int32_t n_reqs, q3tts_result* outs, int16_t** pcm_i16 /* [n_reqs] or NULL */);
int q3tts_node_get_timings(const q3tts_node* n, q3tts_node_timings* out);
const char* q3tts_node_last_error(const q3tts_node* n);
int32_t q3tts_node_size(const q3tts_node* n);
q3tts_engine* q3tts_node_engine(q3tts_node* n, int32_t rank);  /* the engine of device `rank` (sampler defaults, timings); owned by the node */
/* Host only: the global request indices device `rank` of `world` owns, in order ({i : i mod world == rank}); returns the count
 * (idx may be NULL to query it), -1 on bad arguments. */
int32_t q3tts_node_shard(int32_t n_total, int32_t world, int32_t rank, int32_t* idx, int32_t cap);

/* Per-stage device timings of the last generate call (hipEvent), ms. */
typedef struct q3tts_timings {
    float prefill_ms, decode_ms, vocoder_ms, total_ms;
    float frame_step_ms;      /* mean device time of one frame-step graph replay */
    float probe_kernel_ms;    /* q3tts_k_probe: mean in-situ device time of the probed kernel (mode 2: the Talker's layer-0 gate/up GEMM; mode 1: the Predictor's), full batch */
    int64_t frame_steps;      /* graph replays timed */
    int64_t algo_bytes_per_step; /* SURVEY.md §8(d) algorithmic bytes of one frame step at the batch run */
    int64_t algo_flops_per_step; /* 2 * (W_T + 15 W_P + 15 h + pj) * mean live utterances per step (decoder GEMMs) */
    float mean_live_slots;       /* utterances generating, averaged over the timed frame steps */
    float mean_rows;             /* decode rows per frame step (row bucket), averaged over the timed frame steps */
    int64_t probe_count;         /* launches behind probe_kernel_ms */
    float probe_empty_ms;        /* mean elapsed time of an EMPTY event bracket on the same stream (event overhead) */
    float mean_ctx_tokens;       /* sum over the live utterances of their Talker context length, averaged over the timed frame steps */
} q3tts_timings;
int q3tts_get_timings(const q3tts_engine* e, q3tts_timings* out);

/* Log-mel front-end of the voice-clone path (replaces SpeakerEncoder::compute_mel, src/models/onnx.rs:166-321): 24 kHz mono
 * f32 in, [n_frames][128] log-mel out (n_fft 1024, hop 256, Slaney mels, the reference's padding rules). */
int32_t q3tts_mel_frames(int64_t n_samples);
int q3tts_mel(q3tts_engine* e, const float* audio, int64_t n_samples, float* out, int32_t cap_frames, int32_t* n_frames);

/* ---- voice-clone encoders (replace AudioEncoder / SpeakerEncoder, src/models/onnx.rs:82-165, and the encoder half of
 * TtsEngine::create_voice_file, src/tts/engine.rs:324-387). The reference runs two ONNX graphs that are not in its
 * repository; the structure here is the model family's (ECAPA-TDNN speaker encoder; SEANet + transformer + split residual
 * VQ codec encoder), every dimension a field, weights seeded-synthetic or read from two GGUF files
 * (q3tts_clone_load below). ------------------------------------------------------------------------------ */
typedef struct q3tts_clone_config {
    /* speaker encoder: log-mel [T][mel_dim] -> [se_dim] */
    int32_t mel_dim;                 /* 128 (fixed by q3tts_mel) */
    int32_t se_channels[5];          /* 512,512,512,512,1536: TDNN, 3 SE-Res2Net blocks, aggregation (= 3 x block width) */
    int32_t se_kernels[5];           /* 5,3,3,3,1 */
    int32_t se_dilations[5];         /* 1,2,3,4,1 */
    int32_t se_attn_channels;        /* 128 */
    int32_t se_res2net_scale;        /* 8 */
    int32_t se_se_channels;          /* 128 */
    int32_t se_dim;                  /* 2048 = model.d_embed ("spk_emb" [1,2048], src/models/onnx.rs:149) */
    /* audio encoder: 24 kHz PCM -> [frames][ae_n_codebooks] */
    int32_t ae_filters;              /* 64 */
    int32_t ae_kernel, ae_res_kernel, ae_last_kernel;   /* 7, 3, 3 */
    int32_t ae_n_ratios; int32_t ae_ratios[4];          /* 4: 4,5,6,8 (x960) */
    int32_t ae_hidden;               /* 512 */
    int32_t ae_n_layer, ae_n_head, ae_head_dim, ae_d_ffn, ae_window;  /* 8, 8, 64, 2048, 250 */
    float ae_rope_theta, ae_ln_eps, ae_layer_scale;     /* 10000, 1e-5, 0.01 */
    int32_t ae_down_stride;          /* 2 (x1920 = one 12.5 Hz frame) */
    int32_t ae_vq_dim;               /* 256 */
    int32_t ae_n_codebooks, ae_codebook_size;           /* 16, 2048 ("audio_codes" [1,frames,16], src/models/onnx.rs:107) */
} q3tts_clone_config;
void q3tts_clone_default_config(q3tts_clone_config* cfg);
/* "load" both encoders into the engine (the reference does so when the two ONNX files exist, src/tts/engine.rs:105-119);
 * weights are generated from cfg.synth_seed of the engine. Calling it again replaces them. */
int q3tts_clone_init(q3tts_engine* e, const q3tts_clone_config* cfg);
/* ---- trained encoder weights from two GGUF files ----
 * qwen3_tts_speaker_encoder.gguf and qwen3_tts_codec_encoder.gguf (the names mirror the reference's onnx/qwen3_tts_speaker_encoder.onnx
 * and onnx/qwen3_tts_codec_encoder.onnx, src/tts/engine.rs:105-119). Each is looked up in weights_dir (the quant directory), else in its
 * parent: one unquantised pair serves every quant directory. Tensor names and layouts are the state_dict keys and PyTorch layouts of the
 * family's modules (transformers' ECAPA_TimeDelayNet; MimiModel's encoder, encoder_transformer, downsample and the two input_proj) plus
 * quantizer.codebook.{q}.weight [codebook_size][vq_dim]; unknown tensors are ignored.
 *
 * q3tts_clone_config_from_dir (host only, no GPU): the encoders' shape from the two files. On entry *cfg holds a complete clone config; on
 * success every field the metadata states is overwritten. Speaker file, A = "q3tts-speaker-encoder" (its general.architecture): A.mel_dim,
 * A.channels / A.kernel_sizes / A.dilations (integer arrays of 5), A.attention_channels -> se_attn_channels, A.res2net_scale,
 * A.se_channels -> se_se_channels, A.embedding_length -> se_dim. Codec file, A = "q3tts-codec-encoder": A.filters, A.kernel_size,
 * A.residual_kernel_size, A.last_kernel_size, A.ratios (integer array of 1..4; its length -> ae_n_ratios), A.embedding_length -> ae_hidden,
 * A.block_count -> ae_n_layer, A.attention.head_count, A.attention.key_length -> ae_head_dim, A.feed_forward_length,
 * A.attention.sliding_window, A.rope.freq_base, A.attention.layer_norm_epsilon, A.down_stride, A.vq_dim, A.n_codebooks, A.codebook_size.
 * Every key is required; ae_layer_scale parametrises only the synthetic generator and is left alone. Cross-checks: the numbers of
 * transformer layers, SEANet stages, codebooks and Res2Net branches, and the shape of every tensor the metadata implies (every
 * convolution's [n][cin][k], the stride convolutions' kernel 2 x ratio, q/k/v/o_proj, fc1, fc2, the codebooks). Errors go to err (err_cap
 * bytes, NUL-terminated; err may be NULL) and leave *cfg unchanged: Q3TTS_ERR_IO for a missing or unreadable file, named (when exactly
 * one of the two is missing the message names that one); Q3TTS_ERR_INVALID otherwise, naming the file and the key or tensor. */
int q3tts_clone_config_from_dir(const char* weights_dir, q3tts_clone_config* cfg, char* err, int32_t err_cap);
/* Where the two files are, by the rule above (host only): the path of each into its buffer of cap bytes, "" for one that is in neither
 * directory. Returns how many were found (0, 1 or 2), or Q3TTS_ERR_INVALID (a NULL argument, a buffer that is too small; the message,
 * with the size needed, goes to q3tts_last_error(NULL)). The one home of the lookup rule: TtsEngine.new decides with it whether to load. */
int q3tts_clone_files_find(const char* weights_dir, char* speaker_path, char* codec_path, int32_t cap);
/* Load both encoders from the two files. weights_dir NULL: the engine's own weights_path (Q3TTS_ERR_STATE if it was created without one).
 * Both files are opened and checked in full on the host before the device is touched: the config comes from them
 * (q3tts_clone_default_config, then q3tts_clone_config_from_dir), must pass the checks q3tts_clone_init applies, and every value must be
 * finite. While it builds, a load holds one matrix's row-major staging copy on the device beside the encoders (freed per matrix), so its
 * peak is that of q3tts_clone_init plus the largest matrix in bf16. A refusal (Q3TTS_ERR_IO for a file that is not found; Q3TTS_ERR_INVALID for a missing tensor, a shape that disagrees with the
 * metadata, a missing or mistyped key, an unsupported tensor type, a value that is not finite, a file that ends early, a refused config)
 * names the file and the tensor or key and leaves the engine and the encoders it had as they were. Then the encoders are built through
 * the creation path of q3tts_clone_init, each array taken from the file instead of the generator: convolution and projection matrices
 * rounded to bf16 (nearest even; a BF16 container passes bit for bit), biases, LayerNorm, LayerScale and codebooks f32 as stored.
 * Calling it or q3tts_clone_init again replaces the encoders. Refused while a session is open, like q3tts_clone_init; a session clones
 * with whatever was loaded before it opened. */
int q3tts_clone_load(q3tts_engine* e, const char* weights_dir);
/* Where the clone encoders' weights came from: 0 = not loaded, 1 = the seeded synthetic generator (q3tts_clone_init), 2 = the two files
 * (q3tts_clone_load). Codes and embeddings of an engine that answers 1 are the output of random filters. */
int q3tts_get_clone_source(const q3tts_engine* e, int32_t* source);
/* Host-only test hook: the array q3tts_clone_load would upload from the pair found from weights_dir for the synthetic generator's tensor
 * id (comp, which) of oracle/q3_oracle_clone.c, at the shape *cfg: in device layout, after rounding, as f32 (matrices [n][round512(k *
 * cin)], zero in the padding). out may be NULL to query *n. Needs no GPU. */
int q3tts_k_clone_file_tensor(const char* weights_dir, const q3tts_clone_config* cfg, int32_t comp, int32_t which, float* out, int64_t cap,
                              int64_t* n);
/* Host-only test hook: the host half of q3tts_clone_load on the pair found from weights_dir (open, shape, cross-checks, finite values, the
 * config checks of q3tts_clone_init), with its status; the message goes to q3tts_last_error(NULL). Needs no GPU. */
int q3tts_k_clone_load_check(const char* weights_dir);
/* frames the audio encoder produces for n_samples (ceil division through every stride) */
int32_t q3tts_clone_audio_frames(const q3tts_engine* e, int64_t n_samples);
/* AudioEncoder::encode (src/models/onnx.rs:96-121): codes [n_frames][ae_n_codebooks] i64, row-major like "audio_codes".
 * Q3TTS_ERR_STATE with "AudioEncoder not loaded" before q3tts_clone_init (src/tts/engine.rs:330-332). */
int q3tts_clone_audio_encode(q3tts_engine* e, const float* audio, int64_t n_samples, int64_t* codes, int32_t cap_frames,
                             int32_t* n_frames);
/* SpeakerEncoder::encode (src/models/onnx.rs:135-160): log-mel on the device, then the encoder; out [se_dim] */
int q3tts_clone_speaker_encode(q3tts_engine* e, const float* audio, int64_t n_samples, float* spk_emb);
/* test hooks: the speaker encoder on a given log-mel; the audio encoder's pre-quantiser rows [n_frames][ae_hidden] */
int q3tts_k_speaker_from_mel(q3tts_engine* e, const float* mel, int32_t n_frames, float* spk_emb);
int q3tts_k_audio_latent(q3tts_engine* e, const float* audio, int64_t n_samples, float* latent, int32_t cap_frames,
                         int32_t* n_frames);
/* test hook: the audio encoder's split residual VQ alone, on given operands (no engine). ps / pa [T][D] f32 (the semantic / acoustic
 * projections; pa may be NULL when ncb == 1), books row-major [ncb][CS][D] f32; the production codebook transpose and quantiser kernels
 * run once; codes [T][ncb]. D a multiple of 16 in 16 .. 4096, ncb 1 .. 64. */
int q3tts_k_rvq(int32_t device, const float* ps, const float* pa, int32_t T, int32_t D, const float* books, int32_t ncb, int32_t CS,
                int64_t* codes);

/* ---- tokenizer (host only; replaces the `tokenizers`-crate wrapper src/utils/tokenizer.rs:1-37 for non-Rust hosts) ----
 * Reads model_dir/tokenizer/tokenizer.json of the Qwen2 family: added tokens, NFC, Split(Qwen2 regex) + ByteLevel, BPE.
 * Any other pipeline is refused at load (Q3TTS_ERR_UNSUPPORTED); input must be valid UTF-8.
 * No engine and no GPU needed; errors go to the caller's buffer. A handle is not thread-safe (it caches words). */
typedef struct q3tts_tokenizer q3tts_tokenizer;
int q3tts_tokenizer_load(const char* tokenizer_json_path, q3tts_tokenizer** out, char* err, int32_t err_cap);
void q3tts_tokenizer_free(q3tts_tokenizer* t);
int32_t q3tts_tokenizer_vocab_size(const q3tts_tokenizer* t);
/* Tokenizer::encode(text) = inner.encode(text, add_special_tokens = false).get_ids() (src/utils/tokenizer.rs:17-25).
 * *n_ids receives the count even when cap is too small (then Q3TTS_ERR_INVALID). */
int q3tts_tokenizer_encode(const q3tts_tokenizer* t, const char* utf8, int64_t n_bytes, uint32_t* ids, int32_t cap,
                           int32_t* n_ids, char* err, int32_t err_cap);
/* Tokenizer::decode(ids) = inner.decode(ids, skip_special_tokens = false) (:27-35), as raw bytes (the crate applies
 * from_utf8_lossy on top) */
int q3tts_tokenizer_decode(const q3tts_tokenizer* t, const uint32_t* ids, int32_t n, char* out, int64_t cap, int64_t* n_bytes,
                           char* err, int32_t err_cap);

/* ---- kernel-level test hooks (host buffers in/out; used only by tests/ and bench.py) ----------- */
/* y[B][N] = exact_gemm(norm?(x)[B][K], W[N][K] bf16 bits) (+bias) — canonical order of DESIGN.md §4.1 */
int q3tts_k_gemm_exact(int32_t device, const float* x, int32_t B, int32_t K, const uint16_t* w_bf16, int32_t N,
                       const float* norm_w /*NULL: no RMSNorm*/, float eps, const float* bias /*NULL*/,
                       int32_t epilogue /*0 store,1 residual(y+=),2 swiglu,3 argmax*/, float* y, uint64_t* argmax_keys,
                       int32_t iters, float* mean_kernel_ms);
/* fused q/k RMSNorm + RoPE + KV append + decode attention for rows of ONE sequence processed in order */
int q3tts_k_attention(int32_t device, const float* qkv /*[n][(Hq+2Hkv)*hd]*/, int32_t n_rows, int32_t pos0,
                      int32_t n_head, int32_t n_kv_head, int32_t head_dim, const float* q_norm_w, const float* k_norm_w,
                      float eps, float rope_theta, const int32_t* mrope_sections, float* out /*[n][Hq*hd]*/);
/* decode attention as the frame step runs it: per slot, rows 0 .. lens[s] - 2 of qkv (the slots' rows back to back) prepared into a
 * cache of n_ctx positions, then ONE fused decode launch at pos = lens[s] - 1 under decode policy `policy` (-1: the current one, as in
 * q3tts_k_attend_policy); out_f32 [n_slots][Hq*hd]; out_bf16 (optional) the bf16 operand the same launch writes for the O projection */
int q3tts_k_attention_decode(int32_t device, const float* qkv, int32_t n_slots, const int32_t* lens, int32_t n_ctx, int32_t n_head,
                             int32_t n_kv_head, int32_t head_dim, const float* q_norm_w, const float* k_norm_w, float eps, float rope_theta,
                             const int32_t* mrope_sections, int32_t policy, float* out_f32, uint16_t* out_bf16);
/* The attention hooks below reach every kernel of csrc/q3_attend.hip with every output form, and return the cache. Shared by the three:
 *   out_form 0: out = f32 rows [rows][Hq*hd]; 1: out = the bf16 operand of the O projection as bit patterns [rows][Hq*hd] (untiled here);
 *   2: out = int8 quants [rows][Hq*hd] and out_scale = f32 block scales [rows][Hq*hd/32] of the Q8_0 blocks a W8A8 engine's launch writes.
 *   k_cache / v_cache (optional): the cache of every slot after the launch, un-blocked, as bf16 bits [slot][n_kv_head][n_ctx][hd].
 * Every argument is checked on the host — head_dim 128, n_ctx a multiple of 64, the GQA ratio, every length and pos0 + n <= n_ctx — and a
 * bad one returns Q3TTS_ERR_INVALID with nothing launched. */
/* Whole prompt runs as the engine's admission launches them: run i (slot i) has run_pos0[i] rows that k_qk_prep puts into the cache (they
 * stand for a voice prefix) and then run_n[i] rows at positions run_pos0[i] ..; qkv holds run 0's run_pos0[0] + run_n[0] rows, then run
 * 1's, ... The runs' rows go through k_qk_prep and ONE non-fused attention launch that carries the run table, under prefill policy
 * `policy` (-1: the current one; 0 / 1 / 2 as in q3tts_k_attend_policy). out rows: the runs' rows back to back ([sum run_n]). */
int q3tts_k_attention_runs(int32_t device, const float* qkv, int32_t n_runs, const int32_t* run_n, const int32_t* run_pos0, int32_t n_ctx,
                           int32_t n_head, int32_t n_kv_head, int32_t head_dim, const float* q_norm_w, const float* k_norm_w, float eps,
                           float rope_theta, const int32_t* mrope_sections, int32_t policy, int32_t out_form, void* out, float* out_scale,
                           uint16_t* k_cache, uint16_t* v_cache);
/* q3tts_k_attention_decode with one output form per call and the cache; row_indexed = 1: the Predictor's addressing (no row tables:
 * slot = row % n_slots, every slot at the same length lens[0]). out rows: [n_slots]. */
int q3tts_k_attention_decode_ex(int32_t device, const float* qkv, int32_t n_slots, const int32_t* lens, int32_t n_ctx, int32_t n_head,
                                int32_t n_kv_head, int32_t head_dim, const float* q_norm_w, const float* k_norm_w, float eps,
                                float rope_theta, const int32_t* mrope_sections, int32_t policy, int32_t row_indexed, int32_t out_form,
                                void* out, float* out_scale, uint16_t* k_cache, uint16_t* v_cache);
/* The Predictor's pass A (k_attend_pair): qkv [2 * n_slots] rows — row b at position 0 and row n_slots + b at position 1 of slot b — in one
 * launch on an empty cache; two query heads per KV head. out rows: [2 * n_slots], in the same order. */
int q3tts_k_attention_pair(int32_t device, const float* qkv, int32_t n_slots, int32_t n_ctx, int32_t n_head, int32_t n_kv_head,
                           int32_t head_dim, const float* q_norm_w, const float* k_norm_w, float eps, float rope_theta,
                           const int32_t* mrope_sections, int32_t out_form, void* out, float* out_scale, uint16_t* k_cache, uint16_t* v_cache);
/* Host only: the kernel the attention launcher takes for a shape under the current policies, without launching. fused 0 (rows of runs), 1
 * (one row per slot) or 2 (pass A); n_seg = 0: a launch without a run table. *kernel = 0 / 1 / 2: k_attend<1 / 2 / 4, false>; 3 / 4:
 * k_attend<2 / 4, true>; 5: k_attend_gqa2; 6: k_attend_small<2>; 7: k_attend_pair; 8: k_attend_prefill; -1: the launcher refuses. */
int q3tts_k_attend_pick(int32_t fused, int32_t gqa_ratio, int32_t n_ctx, int32_t n_seg, int32_t seg_max_n, int32_t seg_max_t,
                        int32_t n_kv_head, int32_t* kernel);
/* ---- the same over a Q8_0 cache (q3tts_engine_config.kv_q8_0; csrc/q3_attend_kv8.hip) ----
 * q3tts_k_attention_runs / q3tts_k_attention_decode_ex (without row_indexed) with the launch's cache in Q8_0 blocks: the quantising append
 * k_qk_prep_kv8 for the rows that are only cached, then ONE launch through the engine's launcher. The cache comes back un-blocked:
 * k_q / v_q int8 [slot][n_kv_head][n_ctx][hd], k_d / v_d f16 bits [slot][n_kv_head][n_ctx][hd / 32] (each optional). Arguments are
 * checked on the host as above. */
int q3tts_k_attention_runs_kv8(int32_t device, const float* qkv, int32_t n_runs, const int32_t* run_n, const int32_t* run_pos0, int32_t n_ctx,
                               int32_t n_head, int32_t n_kv_head, int32_t head_dim, const float* q_norm_w, const float* k_norm_w, float eps,
                               float rope_theta, const int32_t* mrope_sections, int32_t policy, int32_t out_form, void* out, float* out_scale,
                               int8_t* k_q, int8_t* v_q, uint16_t* k_d, uint16_t* v_d);
int q3tts_k_attention_decode_kv8(int32_t device, const float* qkv, int32_t n_slots, const int32_t* lens, int32_t n_ctx, int32_t n_head,
                                 int32_t n_kv_head, int32_t head_dim, const float* q_norm_w, const float* k_norm_w, float eps,
                                 float rope_theta, const int32_t* mrope_sections, int32_t policy, int32_t out_form, void* out,
                                 float* out_scale, int8_t* k_q, int8_t* v_q, uint16_t* k_d, uint16_t* v_d);
/* Host only: q3tts_k_attend_pick for a launch over a Q8_0 cache. *kernel = 9 / 10 / 11: k_attend_kv8<1 / 2 / 4, false>; 12 / 13:
 * k_attend_kv8<2 / 4, true>; 14: k_attend_gqa2_kv8 (decode policy 0; policy 1 gives 12); -1: the launcher refuses (fused = 2, a fused
 * launch with one query head per KV head, a GQA ratio outside 1, 2, 4). Never 0 .. 8: there is no Q8 form of k_attend_prefill. */
int q3tts_k_attend_pick_kv8(int32_t fused, int32_t gqa_ratio, int32_t n_ctx, int32_t n_seg, int32_t seg_max_n, int32_t seg_max_t,
                            int32_t n_kv_head, int32_t* kernel);
/* ---- the Predictor's layer-0 QKV table ----
 * With a bf16 Predictor and greedy heads, block 0 of passes q = 1 .. n_codebooks - 2 reads its raw q / k / v from a table built at engine
 * creation (one row per (q, code), + one fallback row per q for a code outside [0, codecq_rows)) instead of launching k_pred_next(q) and
 * the QKV GEMM. Environment, read at engine creation: Q3TTS_PRED_TABLE=0 builds no table; Q3TTS_PRED_TABLE_MAX_MB (default 1024): a
 * larger table is not built. Without a table the frame step is the one with those launches; the ids are the same either way.
 * Row `code` of slice q: n_head * head_dim + 2 * n_kv_head * head_dim f32 of the Predictor. Q3TTS_ERR_STATE: the engine has no table. */
int q3tts_k_pred_table_row(q3tts_engine* e, int32_t q, int32_t code, float* out);
/* What one k_pred_next(q) launch of the greedy frame step, 1 <= q <= n_codebooks - 2, works on; row b stands for slot b. codes, fb and px
 * are read and written back: codes[b][n_frames[b]][q] = code, fb[b] += codec_q[code] (+ 0 when the code is outside [0, rows_q)),
 * px[b] = pproj_q[code] (proj_b then). A row with active[b] = 0 is left alone. code = the column of the largest key of keys[b][...]. */
typedef struct q3tts_k_pred_step {
    int32_t n_rows, q, n_codebooks, n_key_parts, rows_q, d_embed, d_proj, max_steps_cap;
    const uint64_t* keys;      /* [n_rows][n_key_parts] */
    const int32_t* active;     /* [n_rows] */
    const int32_t* n_frames;   /* [n_rows], each in [0, max_steps_cap) */
    const float* codec_q;      /* [rows_q][d_embed] */
    const float* pproj_q;      /* [rows_q][d_proj] */
    const float* proj_b;       /* [d_proj] */
    float* fb;                 /* [n_rows][d_embed] */
    float* px;                 /* [n_rows][d_proj] */
    int32_t* codes;            /* [n_rows][max_steps_cap][n_codebooks] */
} q3tts_k_pred_step;
/* k_pred_next<false>(q) on st; also the norm inputs it writes for norm_w [d_proj]: xb bf16 bits [n_rows][d_proj] (natural order; rows of
 * inactive slots stay zero), ssp [n_rows][d_proj / 16]. */
int q3tts_k_pred_next(int32_t device, q3tts_k_pred_step* st, const float* norm_w, uint16_t* xb, float* ssp);
/* One launch of the gathering form of k_attend_small<2> as block 0 of pass st->q issues it: row b (slot b at position len - 1 of the
 * Predictor's row-indexed cache, n_ctx = 64) takes its q / k / v from table[code] (table [rows_q + 1][ld], ld = (n_head + 2 n_kv_head) *
 * head_dim; row rows_q = the fallback row) and one more workgroup column does st's bookkeeping. qkv: n_rows runs of len rows as
 * q3tts_k_attention_decode_ex takes them: the first len - 1 of a run fill the slot's cache, the last one is not read. Outputs as there. */
int q3tts_k_attention_gather(int32_t device, q3tts_k_pred_step* st, const float* table, const float* qkv, int32_t len, int32_t n_ctx,
                             int32_t n_head, int32_t n_kv_head, int32_t head_dim, const float* q_norm_w, const float* k_norm_w, float eps,
                             float rope_theta, const int32_t* mrope_sections, int32_t out_form, void* out, float* out_scale,
                             uint16_t* k_cache, uint16_t* v_cache);
/* sampler (H4: src/models/llama/mod.rs:666-772) on n rows of logits; r_uniform[n] are the f32 draws */
int q3tts_k_sample(int32_t device, const float* logits, int32_t n, int32_t ld, int32_t limit, float temperature,
                   int32_t top_k, float top_p, const float* r_uniform, int32_t* out_ids);
/* Talker forward over a prompt: hidden[d] (post final norm) and logits[t_vocab] of the LAST row */
int q3tts_k_talker_prefill(q3tts_engine* e, const float* embd, int32_t n_tok, float* hidden_out, float* logits_out);
/* The same behind a voice prefix: the prompt is the prefix's rows followed by embd [n_tok][d_embed] */
int q3tts_k_talker_prefill_prefix(q3tts_engine* e, const q3tts_prefix* prefix, const float* embd, int32_t n_tok, float* hidden_out,
                                  float* logits_out);
/* A ready prefix's K store and V store as bytes, zero padding included: *bytes receives the size of each (k = v = NULL only asks for it);
 * cap = bytes each of k / v holds. Refused while a session is open on the prefix's engine. */
int q3tts_k_prefix_read(const q3tts_prefix* x, void* k, void* v, int64_t cap, int64_t* bytes);
/* Vocoder: codes [n_frames][n_codebooks] -> pcm; chunk_frames frames per streaming call (0 = one call) */
int q3tts_k_vocoder(q3tts_engine* e, const int32_t* codes, int32_t n_frames, int32_t chunk_frames, float* pcm_out,
                    int32_t* n_samples_out);
/* Vocoder transformer rows: q3tts_k_vocoder's calls on slot 0, and after each the f32 residual rows after the last layer (before the
 * final norm) -> out [n_frames][latent_dim] */
int q3tts_k_vocoder_latent(q3tts_engine* e, const int32_t* codes, int32_t n_frames, int32_t chunk_frames, float* out);
/* Vocoder convolution half, stage by stage: q3tts_k_vocoder's calls on slot 0 (calls of <= 4 frames, numbered from 0); call `tap_call`
 * runs eagerly with named copies of its intermediate tensors taken between the production launches, and the drive ends after it. Each
 * tap is (hist_rows + rows) x channels elements at buf + offset, f32 (dtype 0) or bf16 bits (dtype 1), as plain rows (layout 0) or in
 * the GEMM's A-tiled layout (layout 1: whole 16-row tiles). Names: up<u>.in / .raw / .ln / .gelu / .out (ConvTranspose input, its raw
 * output with the depthwise history, LayerNorm output, GELU output, the stage's result), dec_in.in, b<b>.ct_in, b<b>.o_ct,
 * b<b>.r<u>.c1_in, b<b>.r<u>.z (un-fused path only), b<b>.r<u>.o (u < 2: the last unit's sum is never stored), out.in, pcm.
 * Front half (slot 0's rows of the call): emb (the pre-conv's input: the codebook sums behind pre_conv_kernel - 1 history rows), x0 (the
 * pre-conv's output), per transformer layer l: l<l>.xn (input norm, bf16), l<l>.qkv (q | k | v before RoPE, f32), l<l>.kring / l<l>.vring
 * (slot 0's whole ring after the attention launch: sliding_window + 4 rows of n_head * head_dim, position p in row p % rows; rotated keys),
 * l<l>.att (bf16), l<l>.x_att (the residual rows after the attention branch), l<l>.xn2 (post norm, bf16), l<l>.g (SwiGLU output, bf16),
 * l<l>.x_out (the residual rows after the MLP branch); final.xn (the final norm: f32, or A-tiled bf16 where the up-sampling GEMMs read that). */
typedef struct q3tts_voc_tap {
    char name[32];
    int32_t dtype, layout, hist_rows, rows, channels, reserved;
    uint64_t offset;
} q3tts_voc_tap;
int q3tts_k_vocoder_taps(q3tts_engine* e, const int32_t* codes, int32_t n_frames, int32_t chunk_frames, int32_t tap_call, void* buf,
                         uint64_t buf_bytes, q3tts_voc_tap* recs, int32_t rec_cap, int32_t* n_recs);
/* Host-only: the array q3tts_engine_create would upload from the vocoder file `path` for the synthetic generator's tensor id (comp,
 * which) of oracle/q3_oracle_vocoder.c, at the shape *vc: in device layout, after rounding (bf16-representable where the device holds
 * bf16), as f32; for a SnakeBeta id the evaluated exp(alpha) / 1 / (exp(beta) + 1e-9). out may be NULL to query *n. Needs no GPU. */
int q3tts_k_voc_file_tensor(const char* path, const q3tts_vocoder_config* vc, int32_t comp, int32_t which, float* out, int64_t cap, int64_t* n);
/* Measurement (bench.py roofline_vocoder): the batched vocoder alone, n_slots slots x `chunks` 4-frame calls with nothing else on the
 * GPU; *ms_per_chunk = mean duration of one batched call (n_slots x 4 frames of PCM) by HIP events on its stream. */
int q3tts_k_vocoder_bench(q3tts_engine* e, int32_t n_slots, int32_t chunks, float* ms_per_chunk);
/* Host-only: one tensor of a GGUF file (or the array of an .npy file; `tensor` is then ignored) as f32, through the same
 * reader the engine uses for weights_path. out may be NULL to query nelem / dims (ggml order: dims4[0] is the row length)
 * / ggml type (0 F32, 1 F16, 8 Q8_0, 30 BF16). Needs no GPU. */
int q3tts_k_gguf_read(const char* path, const char* tensor, float* out, int64_t cap, int64_t* nelem, int64_t* dims4, int32_t* ggml_type);
/* Host-only: one metadata value of a GGUF file through the same reader. *value_type = the GGUF value type (0 u8, 1 i8, 2 u16, 3 i16,
 * 4 u32, 5 i32, 6 f32, 7 bool, 8 string, 9 array, 10 u64, 11 i64, 12 f64), *elem_type = an array's element type (else the value type),
 * *count = an array's length (else 1). Numbers (scalars and arrays) go to values as doubles (values_cap elements). A string's bytes go to
 * str (str_cap bytes, no terminator), *str_bytes = their count; a string array's elements go to str as the file stores them (each a
 * little-endian u64 length, then its bytes). values / str may be NULL to query types, count and *str_bytes. A missing key is
 * Q3TTS_ERR_INVALID. Needs no GPU. */
int q3tts_k_gguf_meta(const char* path, const char* key, int32_t* value_type, int32_t* elem_type, int64_t* count, double* values,
                      int64_t values_cap, char* str, int64_t str_cap, int64_t* str_bytes);
/* Measurement mode for bench.py: frame steps are launched eagerly (no graph replay) and ONE launch of every frame is bracketed
 * by HIP events on its own stream. enable = model + 16 * kind; model 2: block 0 of the Talker step, model 1: block 0 of the
 * Predictor's pass 1; kind 0: the gate/up GEMM (so enable = 2 / 1 are the Talker's / Predictor's gate/up as before), 1: QKV GEMM,
 * 2: attention kernel, 3: O projection, 4: down projection. q3tts_timings.probe_kernel_ms / probe_count report it for the frame
 * steps that ran at the full row count. enable = 0 restores graph replay. */
int q3tts_k_probe(q3tts_engine* e, int32_t enable);
/* n_cases independent chains of `chain` v_mfma_f32_16x16x32_bf16 into one accumulator tile: a [n][chain][16][32] bf16 bits,
 * b [n][chain][32][16], c / d [n][16][16] f32. Pins the instruction's accumulation arithmetic. */
int q3tts_k_mfma_bf16(int32_t device, const uint16_t* a, const uint16_t* b, const float* c, float* d, int32_t n_cases, int32_t chain);
/* The decoder's GEMM as the engine launches it (csrc/q3_bgemm.hip): bf16 rows xb [B][K] x W [N][K] (bf16 bit
 * patterns, row-major; tiled on the device) on v_mfma_f32_16x16x32_bf16, K % 256 == 0, N % 16 == 0. ssp [B][ntiles] (or NULL) are
 * the producer's per-tile sums of squares: s_r = 1 / sqrtf(SS(ssp) / d_norm + eps).
 *   epilogue 0: y[B][N] = s_r * RAW            1: y += RAW (y in/out); with nw_next[N] also yb[B][N] = bf16(y * nw_next), ssp_out[B][N/16]
 *            2: yb[B][N/2] = bf16(swiglu(s_r * RAW_gate, s_r * RAW_up)), W = the N/2 gate rows then the N/2 up rows
 *            3: keys[B] = argmax key over s_r * RAW
 * Equals oracle q3o_bgemm bit for bit for every row count (the tile shape the launcher picks never changes a result). */
int q3tts_k_bgemm(int32_t device, const uint16_t* xb, int32_t B, int32_t K, const uint16_t* w_bf16, int32_t N, const float* ssp, int32_t ntiles,
                  int32_t d_norm, float eps, int32_t epilogue, const float* nw_next, float* y, uint16_t* yb, float* ssp_out, uint64_t* keys,
                  int32_t iters, float* mean_kernel_ms);
/* Which kernel serves launches of >= 256 rows: 1 = the many-row kernel (k_bgemm_big) whenever eligible, -1 = never, 0 = when it fills the
 * chip (default; the environment variable Q3TTS_BG_BIG sets the initial value once per process). The results are the same bits. */
int q3tts_k_bgemm_policy(int32_t big);
/* Which kernel variant serves the Talker's decode attention (0 = k_attend_gqa2, default; 1 = k_attend<2, true>) and the prefill of whole
 * prompts (0 = k_attend_prefill when the launch has >= 128 (run, KV head) workgroups, default; 1 = never: k_attend<2, false>; 2 = whenever
 * eligible). Same bits either way (tests compare them in one process); Q3TTS_ATT_OLD / Q3TTS_ATT_PREFILL_OLD set the initial values. */
int q3tts_k_attend_policy(int32_t decode, int32_t prefill);
/* force = 1: the frame step runs its sampling form (the Predictor's heads store their logits, k_pred_next<true> picks from them) whatever the
 * Predictor sampler's temperature; at temperature 0 that is sample_row's greedy branch, which must give the ids of the default form (the
 * heads' ARGMAX epilogue). 0: back to the rule (sampling form iff temperature > 0). Q3TTS_ERR_STATE while a session or a stream is open. */
int q3tts_k_pred_variant(q3tts_engine* e, int32_t force);
/* The readiness rule of "streaming text input" as the session worker applies it: 1 iff a request with n_text text ids so far (x, the
 * first one included), closed or not, at n_frames frames may take part in the next chunk of 4 frame steps. Needs no GPU. */
int q3tts_k_text_ready(int32_t n_text, int32_t closed, int32_t n_frames);
/* The credit rule of "paced requests and swapping" as the session worker applies it: 1 iff a paced request with that credit at n_frames
 * frames may take the next chunk of 4 frame steps (n_frames + 4 <= credit; a negative credit is a lifted limit). Needs no GPU. */
int q3tts_k_credit_ready(int64_t credit, int32_t n_frames);
/* The rules of a well-formed request that every entry refuses alike (sessions at submit, every admission): text_open needs text_stream;
 * text_stream needs a prompt built from ids with n_text >= 1; with keep != 0 (the request's voice is to be kept as a prefix, keep_rows =
 * voice_rows) it names no prefix and states voice_rows >= 1 with prompt_embd, >= 0 with a prompt. Q3TTS_OK, or Q3TTS_ERR_INVALID (a NULL
 * request too) with the rule named in msg, a string of at most cap - 1 characters (msg may be NULL). Needs no GPU. */
int q3tts_k_request_rules(const q3tts_request* r, int32_t keep, int32_t keep_rows, char* msg, int32_t cap);
/* The swap arena's allocator alone (host only): ops[0, n) replayed over an arena of cap bytes. ops[i] > 0 allocates that many bytes:
 * offsets[i] = the block's offset (a multiple of 256), or -1 for "no room". ops[i] = -(k + 1) frees what ops[k] allocated (k < i, a live
 * allocation): offsets[i] = the freed offset. Anything else is Q3TTS_ERR_INVALID. */
int q3tts_k_swap_arena(int64_t cap, const int64_t* ops, int32_t n, int64_t* offsets);
/* Measurement hook (tools/paced_bench.py): the worker's HOST wall time in the two swap phases of its chunk boundaries so far, counted
 * over the boundaries that moved at least one block: out[0] ms in swap_out, out[1] ms in swap_in (launches, the host waits for a target
 * slot's previous occupant, the text upload's synchronise), out[2] the number of such boundaries. The copies themselves run on the two
 * streams behind these phases and are not in it. Q3TTS_ERR_INVALID for a NULL session ("null session") or a NULL out. */
int q3tts_k_swap_phase_ms(const q3tts_session* s, double out[3]);
/* The k_bgemm instance the launcher takes for a shape, without launching: out5 = {row tiles, column tiles, ring depth, non-temporal weight
 * loads, 1 if k_bgemm_big}. bench.py names the kernel symbol of a probed launch from it. */
int q3tts_k_bgemm_pick(int32_t B, int32_t K, int32_t N, int32_t epilogue, int32_t w_once, int32_t q8, int32_t* out5);
/* The same launch with ggml Q8_0 weights kept in block form on the device: q int8 [N][K] row-major (epilogue 2: the
 * N/2 gate rows, then the N/2 up rows), d_f16 the blocks' f16 scales as bit patterns [N][K/32]; K % 512 == 0. Equals oracle q3o_bgemm_q8
 * bit for bit. */
int q3tts_k_bgemm_q8(int32_t device, const uint16_t* xb, int32_t B, int32_t K, const int8_t* q, const uint16_t* d_f16, int32_t N, const float* ssp,
                     int32_t ntiles, int32_t d_norm, float eps, int32_t epilogue, const float* nw_next, float* y, uint16_t* yb, float* ssp_out,
                     uint64_t* keys, int32_t iters, float* mean_kernel_ms);
/* The same launch in ggml's Q8_0 x Q8_0 arithmetic (W8A8: csrc/q3_bgemm8.hip; q3tts_engine_config.talker_q8_0 = 2): the
 * ACTIVATIONS are Q8_0 blocks too — aq int8 [B][K], ad their block scales as f32 [B][K/32] (the producers store d = amax / 127 rounded to
 * f16's 11-bit significand but kept in f32; any f32 is accepted) — a block's product is its exact int32 sum times f32(d_w) * d_x. epilogue 0: y = s_r * RAW; 1: y += RAW, then the consumer's operand v = y * nw_next quantised per 32
 * columns by ggml's rule -> yq int8 [B][N], yd f32 [B][N/32], and ssp_out; 2: h = swiglu(s_r * RAW_gate, s_r * RAW_up) quantised ->
 * yq [B][N/2], yd [B][N/64]. K % 512 == 0; N % 32 == 0 (1: % 64, 2: % 128). Equals oracle q3o_bgemm_q8a8_f32 bit for bit. */
int q3tts_k_bgemm_q8a8(int32_t device, const int8_t* aq, const float* ad, int32_t B, int32_t K, const int8_t* q, const uint16_t* d_f16, int32_t N,
                       const float* ssp, int32_t ntiles, int32_t d_norm, float eps, int32_t epilogue, const float* nw_next, float* y, int8_t* yq,
                       float* yd, float* ssp_out, int32_t iters, float* mean_kernel_ms);
/* The same launch with epilogue 3 (ARGMAX: the heads of a Predictor with predictor_q8_0 = 2): per-tile maxima keys over s_r * RAW, reduced as
 * k_pred_next reduces them (the row's largest key; of equal logits the lower column wins) -> ids_out[B] = the winning column of each row.
 * ssp may be NULL (no row scale). Equals np.argmax of oracle q3o_bgemm_q8a8_f32 (epilogue 0) per row. */
int q3tts_k_bgemm_q8a8_argmax(int32_t device, const int8_t* aq, const float* ad, int32_t B, int32_t K, const int8_t* q, const uint16_t* d_f16, int32_t N,
                              const float* ssp, int32_t ntiles, int32_t d_norm, float eps, int32_t* ids_out);
/* The same GEMM with the epilogue extras only the vocoder uses (nothing in the reference: its vocoder is an ONNX graph, src/models/onnx.rs:342-459):
 * bias[col % bias_n] added to RAW first; epilogue 0: y = RAW + bias; 1: y += col_scale[col] * (RAW + bias), optionally yb = bf16(y);
 * 4: yb = bf16(gelu_erf(RAW + bias)). seg_rows > 0: the f32 rows live in B / seg_rows segments separated by gap_rows rows the kernel
 * must not touch (checked by the hook). y / yb are dense [B][N] on the host side. */
int q3tts_k_bgemm_voc(int32_t device, const uint16_t* xb, int32_t B, int32_t K, const uint16_t* w_bf16, int32_t N, int32_t epilogue, const float* bias,
                      int32_t bias_n, const float* col_scale, int32_t seg_rows, int32_t gap_rows, float* y, uint16_t* yb, int32_t want_yb);
/* H6 — Assets::project (src/assets_manager.rs:383-399) in the reference's own f32 sequence: y[r][o] = bias[o]; y += x[r][i] * w[o][i]
 * for i ascending (w f32 row-major [n_out][n_in]). nw != NULL: also the rows' norm inputs xb = bf16(y * nw), ssp [rows][n_out/16]. */
int q3tts_k_project(int32_t device, const float* x, int32_t rows, int32_t n_in, const float* w, const float* bias, int32_t n_out, const float* nw,
                    float* y, uint16_t* xb, float* ssp);
/* producer side of the split RMSNorm for plain f32 rows: xb = bf16(x * nw), ssp[r][t] = sum of squares of tile t */
int q3tts_k_norm_inputs(int32_t device, const float* x, int32_t rows, int32_t d, const float* nw, uint16_t* xb, float* ssp);
/* Allocator contract: device memory is handed out with its zero fill COMPLETED. Allocates `bytes` through the engine's allocator,
 * uploads a pattern into the first and last 4 KiB on the null stream at once, and reports the bytes that read back wrong (0 expected). */
int q3tts_k_alloc_upload(q3tts_engine* e, int64_t bytes, int64_t* mismatches);
/* The PCM gather of sessions and of the node's i16 gather (one launch): entry j copies src[row_j][first_j, first_j + count_j) to
 * out[dst_j, dst_j + count_j); src is [rows][stride] f32 (uploaded to a fresh device buffer), n_ent <= 64; format 0: f32 out, 1: i16 by
 * the reference's WAV rule. Windows outside src or out (out_n samples) are refused. */
int q3tts_k_pcm_pack(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* ent_row, const int32_t* ent_first,
                     const int32_t* ent_count, const int64_t* ent_dst, int32_t n_ent, int32_t format, void* out, int64_t out_n);
/* The resampler's coefficient table, host only (no GPU needed): L, M, H of the pair and tab[p][k], L x (2H + 1) values
 * computed in double and rounded once to f32; *n = L x (2H + 1) (cap too small: Q3TTS_ERR_INVALID with L, M, H and *n set). */
int q3tts_k_resample_table(int32_t rate_in, int32_t rate_out, int32_t* L, int32_t* M, int32_t* H, float* tab, int64_t cap, int64_t* n);
/* The resampling sibling of q3tts_k_pcm_pack (one launch): row r of src [rows][stride] holds row_len[r] valid samples at rate_in (what
 * lies beyond is never loaded) and is finished or not (row_final[r]); entry j writes outputs [first_j, first_j + count_j) of its row AT
 * rate_out to out[dst_j, ...). A window past what the row can deliver (N of its length when final, D otherwise) is refused.
 * iters > 0 and mean_ms != NULL: the launch is repeated iters times between two events and *mean_ms receives the mean. */
int q3tts_k_pcm_resample(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* row_len, const int32_t* row_final,
                         const int32_t* ent_row, const int32_t* ent_first, const int32_t* ent_count, const int64_t* ent_dst, int32_t n_ent,
                         int32_t rate_in, int32_t rate_out, int32_t format, void* out, int64_t out_n, int32_t iters, float* mean_ms);
/* N_t(n) and D_t(n) of the time-stretch at `permille` (500..2000), as the engine's host code computes them. Needs no GPU. */
int q3tts_k_tempo_counts(int64_t n, int32_t permille, int64_t* N, int64_t* D);
/* The time-stretch kernel through the engine's launcher: src [rows][stride] f32; step t of n_steps makes one launch (per 64 rows) with
 * row r's valid length lens[t * rows + r] (ascending in t; what lies beyond is never loaded), finished in the last step where
 * row_final[r]. out [n_steps][rows][out_stride] receives the whole output rows after every step (what no launch has written is NaN),
 * n_valid [n_steps][rows] the outputs a row holds then (N_t or D_t), delta [rows][delta_stride] (delta_stride > 0) every decided frame's
 * d_k. iters > 0 and mean_ms != NULL: the last step's launches are repeated iters times between two events and *mean_ms receives the mean. */
int q3tts_k_pcm_tempo(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* lens, int32_t n_steps, const int32_t* row_final,
                      int32_t permille, float* out, int64_t out_stride, int32_t* n_valid, int32_t* delta, int64_t delta_stride, int32_t iters, float* mean_ms);
/* The row buckets of an engine with max_batch slots, ascending (a frame step runs on the smallest bucket that holds the live slots; one
 * captured graph per bucket): 1, 2, 4, 8, the multiples of 16 up to 64, above 64 the multiples of 32, last max_batch itself. Returns the
 * count (<= cap), Q3TTS_ERR_INVALID for max_batch outside 1..Q3TTS_MAX_BATCH or a cap too small. Needs no GPU. */
int q3tts_k_row_buckets(int32_t max_batch, int32_t* out, int32_t cap);
/* out[i] = the frame steps the engine has run on bucket i of q3tts_k_row_buckets(max_batch) since it was created. Returns the bucket count.
 * The counters are atomic: the hook may be called from any thread while a session's worker runs. */
int q3tts_k_bucket_steps(const q3tts_engine* e, int64_t* out, int32_t cap);
/* out2[0] = k_kv_prefix launches since the engine was created, out2[1] = the most prefixed requests one prefill group has held (a group of
 * more than 64 launches the full 64-entry descriptor and starts another). */
int q3tts_k_prefix_stats(const q3tts_engine* e, int64_t* out2);
/* What q3tts_engine_create compares with the device's free memory before it allocates: the bytes the config alone sizes (weights, the
 * two caches, per-slot decode state, the lane's and the prefill's rows and scratch, the vocoder's PCM rows and attention rings). A lower
 * bound of q3tts_k_device_bytes of the created engine (the tests hold it to that). Needs no GPU. */
int q3tts_k_engine_footprint(const q3tts_engine_config* cfg, int64_t* bytes);
/* Device bytes the engine's one allocator has handed out so far: everything that lives as long as the engine (weights, tables, caches,
 * rows, scratch, the vocoder's weights, work buffers and per-slot state), and the rows of a session's live documents. Not counted: what regrows on demand (device-resident PCM, the
 * resampler's staging, the time-stretch's rows, voice prefixes, a session's staging buffer) and the weight loaders' temporary staging. */
int q3tts_k_device_bytes(const q3tts_engine* e, int64_t* bytes);
/* rand 0.8 StdRng (ChaCha12) stream: seed_from_u64(seed) then n x gen::<f32>() */
int q3tts_k_rng_f32(uint64_t seed, int32_t n, float* out);

/* ---- long documents: split text, run the segments as one batch, join their PCM on the device --------------------
 * A request carries one prompt and ends at max_steps (512 frames, 41 s: the reference's own cap, src/tts/engine.rs:152, where
 * generate_with_voice truncates). A document is cut into segments, every segment runs as a request in one voice through the
 * continuous batch, and a device stage trims, fades and lays the segments' PCM rows out as ONE row, so the audio crosses to the host
 * once, with a table of where every segment landed. The reference has no counterpart. Off unless called: nothing else changes.
 *
 * 1. The splitter (host only: no engine, no GPU). Lengths are UTF-8 BYTES on purpose: a CJK character is 3 bytes and about 0.22 s of
 *    speech, a Latin letter 1 byte and about 0.07 s, so bytes track duration across scripts; 240 bytes are about 17 s, well inside 512
 *    frames. The defaults (target 120, max 240) are first choices that nobody has listened to. Rules, on code points:
 *    - invalid UTF-8: Q3TTS_ERR_INVALID, the message holds the byte offset of the offending sequence. Limits: 16 <= target <= max <= 4096.
 *    - whitespace: U+0020 \t \r \n U+00A0 U+3000. A paragraph break is a whitespace run holding two or more \n (one \n is plain
 *      whitespace: hard-wrapped text does not split).
 *    - terminators . ! ? U+2026 U+3002 U+FF01 U+FF1F; closers " ' ) ] } U+201D U+2019 U+300D U+300F U+FF09 U+3011 U+300B. A sentence
 *      end is a maximal run of terminators plus the maximal run of closers behind it. A run of ASCII terminators only counts when
 *      whitespace or the end of the text follows the closers (3.14 and a.b do not cut). A run that is one lone '.' does not count when
 *      the maximal run of ASCII letters directly before it is a single letter (J. K., e.g.) or, case-insensitively, one of
 *      mr mrs ms dr prof sr jr st vs.
 *    - units: the text is cut after every sentence end (kind SENTENCE) and at every paragraph break (PARAGRAPH); each unit is trimmed of
 *      whitespace; a unit without a \p{L} or \p{N} code point is dropped, and if it ended on a paragraph break that kind moves to the
 *      previous kept unit.
 *    - a unit longer than max_bytes is cut repeatedly, at the first of: after the last clause mark (, ; : followed by whitespace, or
 *      U+FF0C U+3001 U+FF1B U+FF1A) whose end lies in (begin + max / 4, begin + max], kind CLAUSE; at the last whitespace code point that
 *      starts in that range, kind HARD; at the largest code-point boundary <= begin + max, kind HARD. The pieces are trimmed and count as
 *      units from here on; the last one keeps the unit's kind.
 *    - packing: greedy, left to right, never across a PARAGRAPH end: the current span absorbs the next unit iff next.end - cur.begin <=
 *      target_bytes. A span's kind is that of its last unit's end; the last span of the text has kind END.
 *    *n_spans is set even when cap is too small (then Q3TTS_ERR_INVALID, as q3tts_tokenizer_encode). Text with nothing speakable gives
 *    Q3TTS_OK and 0 spans. Errors go to err (always NUL-terminated when err_cap > 0; may be NULL). */
#define Q3TTS_BREAK_END 0        /* last segment of the text */
#define Q3TTS_BREAK_HARD 1       /* forced cut at whitespace or a code-point boundary */
#define Q3TTS_BREAK_CLAUSE 2     /* forced cut after a clause mark */
#define Q3TTS_BREAK_SENTENCE 3
#define Q3TTS_BREAK_PARAGRAPH 4
typedef struct q3tts_text_span { int64_t begin, end; int32_t kind; } q3tts_text_span;   /* byte range of the source */
int q3tts_text_split(const char* utf8, int64_t n_bytes, int32_t target_bytes /*0: 120*/, int32_t max_bytes /*0: 240*/,
                     q3tts_text_span* spans, int32_t cap, int32_t* n_spans, char* err, int32_t err_cap);

/* 2. The join: its arithmetic. All at the vocoder's rate, indices 64-bit. A segment is a device row x_i[0, n_i) plus its break kind.
 *    The block length is the constant W = 240 (10 ms). Every value of q3tts_join_opts and W are quality parameters nobody has heard yet.
 *    - edges: block b covers [bW, min((b + 1)W, n_i)); it is loud iff some sample in it has fabsf(x) > threshold (strict; a NaN is not
 *      loud). trim = 0: lo = 0, hi = n_i. trim = 1 with no loud block: lo = hi = 0, the segment is empty. trim = 1 otherwise, with the
 *      first and last loud block: lo = max(0, first W - keep), hi = min(n_i, (last + 1) W + keep). The measure is a peak magnitude, not an
 *      energy sum, on purpose: there is no summation order to pin.
 *    - piece: L_i = hi - lo, F_i = min(fade, L_i div 2). Sample j of the piece is x_i[lo + j]; for j < F_i it is multiplied by g(j, F_i),
 *      for j >= L_i - F_i by g(L_i - 1 - j, F_i), g(j, F) = (float)(j + 1) / (float)(F + 1), the correctly rounded f32 quotient. The gain
 *      is one rounded f32 multiply; outside the fades the sample is copied bit for bit.
 *    - layout: non-empty pieces in order; between consecutive non-empty pieces a < b lie pause_ms[k] * (rate / 1000) samples of +0.0f
 *      (24 per ms), k the largest break kind of segments a .. b - 1, so a dropped piece cannot swallow a paragraph pause. N is the total;
 *      nothing at or beyond N is written. An empty piece reports begin == end == the end of the last non-empty piece before it (0: none).
 *    Q3TTS_ERR_INVALID for trim outside 0 / 1, a threshold that is negative or NaN, a negative keep or fade, a pause outside 0..60000 ms. */
typedef struct q3tts_join_opts {
    int32_t trim;          /* 1 */
    float threshold;       /* 0.01f */
    int32_t keep;          /* 480 samples */
    int32_t fade;          /* 120 samples */
    int32_t pause_ms[5];   /* by break kind: {0, 0, 150, 300, 600} */
} q3tts_join_opts;

/* 3. The entry points. q3tts_generate_long runs segment i as a request built from: a text-only desc over ids, the prefix, want_pcm = 2,
 *    the template's sampler fields, min_frames and force_eos_at, its own max_steps (0: the template's), and seed_i = tmpl.seed + i
 *    (mod 2^64) when has_seed. use_engine_sampler = 1 is resolved into explicit fields at entry, then the same seed rule applies. The
 *    template's text_stream must be off and its prompt_embd, prompt and prefix NULL. Exactly one of voice (a voice-only desc, n_text == 0:
 *    a prefix is created from it at entry and destroyed at return) and prefix (the caller's own) is given. opts == NULL: the defaults.
 *    All segments go through q3tts_generate_batch's machinery with device PCM switched on for the call: the caller's
 *    q3tts_set_device_pcm state is put back as it was, the device buffer's content is replaced as any call replaces it, the segments are
 *    not copied to the host. There may be more segments than slots; n_segs <= 1024. Device memory: n_segs rows of max_steps_cap x samples
 *    per frame x 4 B plus the document rows (the joined row of at most sum_i max_steps_i x samples per frame + the pauses; with a speed
 *    its stretched row, with a rate its resampled row), checked against the device's free memory first: Q3TTS_ERR_OOM naming both numbers.
 *    Then: the edges, the join, with speed_permille the time-stretch's launch over the document row, with output_rate the resampler's,
 *    one device-to-host copy.
 *    Contract: pcm == q3tts_resample(q3tts_time_stretch(J)) bit for bit, J the join (2.) of the PCM q3tts_generate_batch returns for
 *    the same requests with want_pcm = 1 — by the prefix contract also the join of whole-prompt requests, independent of max_batch, of
 *    slot assignment and of admission order.
 *    Failures: a segment that fails by itself makes the call return that segment's status (the first such); info[i].status is filled for
 *    every segment, pcm is NULL, everything stays freeable. Q3TTS_ERR_STATE while a session or a stream is open, and while an engine-level
 *    speed or output rate is set (q3tts_set_speed / q3tts_set_output_rate are the engine's for plain requests; a document carries its own
 *    in opts). Q3TTS_ERR_INVALID: no vocoder, n_segs outside 1..1024, a break kind outside 0..4, a speed or rate outside the ranges of the
 *    two setters, join options outside theirs, a document of more than 2^28 samples. A refused call leaves every piece of engine state as
 *    it was. q3tts_long_result_free releases pcm (pinned) and info. */
typedef struct q3tts_long_segment { const uint32_t* ids; int32_t n_ids; int32_t kind; int32_t max_steps /*0: the template's*/; } q3tts_long_segment;
typedef struct q3tts_long_opts { q3tts_join_opts join; int32_t speed_permille /*0 or 1000: off*/; int32_t output_rate /*0: native*/; } q3tts_long_opts;
typedef struct q3tts_long_info {   /* one per segment */
    int32_t status, n_frames, hit_eos; int64_t n_native, lo, hi;   /* the segment's own row and its kept range */
    int64_t begin, end;           /* the piece in the joined 24 kHz timeline (begin == end: empty) */
    int64_t out_begin, out_end;   /* the same through the speed and rate maps: ceil(s*1000/speed), then ceil(s*L/M) */
} q3tts_long_info;
typedef struct q3tts_long_result { int32_t status, n_segments, n_truncated /*hit_eos == 0*/, sample_rate; int64_t n_samples; float* pcm /*pinned*/;
    q3tts_long_info* info; float generate_ms, join_ms, total_ms; } q3tts_long_result;
void q3tts_long_default_opts(q3tts_long_opts*);
int q3tts_generate_long(q3tts_engine* e, const q3tts_request* tmpl, const q3tts_prompt_desc* voice, const q3tts_prefix* prefix,
                        const q3tts_long_segment* segs, int32_t n_segs, const q3tts_long_opts* opts, q3tts_long_result* out);
void q3tts_long_result_free(q3tts_long_result*);
/* one-shot join of finished host clips: uploads, the same two kernels, one copy back. n_clips in 1..1024; *n_out = N (cap too small:
 * Q3TTS_ERR_INVALID with *n_out set). opts == NULL: the defaults. */
int q3tts_pcm_join(q3tts_engine* e, const float* const* clips, const int64_t* n, const int32_t* kinds, int32_t n_clips,
                   const q3tts_join_opts* opts, float* out, int64_t cap, int64_t* n_out, int64_t* edges /*[n_clips][4]: lo, hi, begin, end; may be NULL*/);
/* Kernel hooks, one launch each through the engine's launcher. src [rows][stride] f32 is uploaded as it is (the tests put NaN behind every
 * valid length lens[r]: nothing at or past it is loaded). q3tts_k_pcm_edges: edges[r] = {first, last} loud block of row r, {INT32_MAX, -1}
 * when none is. q3tts_k_pcm_join: the plan (lo, hi, begin, end per row, and *N) from such edges, the kinds and opts at `rate` samples per
 * second, then the launch into out [out_cap] (uploaded first, so what the launch does not write keeps its value) and the whole buffer back.
 * iters > 0 and mean_ms != NULL: the launch is repeated iters times between two events and *mean_ms receives the mean. */
int q3tts_k_pcm_edges(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* lens, float threshold, int32_t* edges,
                      int32_t iters, float* mean_ms);
int q3tts_k_pcm_join(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* lens, const int32_t* kinds, const int32_t* edges,
                     const q3tts_join_opts* opts, int32_t rate, float* out, int64_t out_cap, int64_t* plan, int64_t* N, int32_t iters, float* mean_ms);

/* ---- documents in a session: the streaming join --------------------------------------------------------------------
 * q3tts_generate_long returns when the last segment is done, and is refused while a session is open; a session streams every request's
 * chunks but a request ends at max_steps. A DOCUMENT is submitted to an open session as segments (ids, a break kind, max_steps: exactly
 * q3tts_long_segment) and streams in order while later segments still run.
 *
 * The bits. The concatenation of all Q3TTS_EV_CHUNK payloads of a document's id is the pcm q3tts_generate_long returns for the same
 * template, the same voice, the same segments (appended ones included, in order) and the same q3tts_join_opts, speed_permille
 * and output_rate (below): bit for bit, whatever the slot count, `ahead`, the admission order, and whatever plain requests share the
 * session. In an i16 session the chunks are the Q3TTS_PCM_I16 conversion of that row (k_pcm_pack's, applied after the fade's multiply).
 * Where the chunk boundaries of a document fall depends on when its segments found slots: only the concatenation is contract.
 *
 * Submitting. The template's rules are q3tts_generate_long's: use_engine_sampler = 1 is resolved at entry, seed_i = seed + i over the
 * GLOBAL segment index, text_stream off, prompt_embd / prompt / prefix NULL. Exactly one of voice (a voice-only desc: the session makes
 * the prefix as a job of "voices in a session" and releases it when the document ends) and prefix (the caller's, ready or pending) is
 * given. Everything is copied before the call returns. n_segs is 1..1024 per call (0 allowed with open = 1). The id comes from the
 * requests' id space. q3tts_session_document_append adds segments to a document submitted with open = 1 and, with close != 0, ends it;
 * an open document whose segments are all delivered stays open and silent until appended to or closed.
 * Events, all with the document's id: CHUNK (the last one has is_final = 1 and may be empty); Q3TTS_EV_SEGMENT once per segment, in
 * order, when the segment's piece (possibly empty) has been fully handed to the ring: n_samples = the segment's index, result = the
 * segment's own (codes, n_frames, hit_eos; n_samples = the piece's length); DONE once the last segment of a closed document is
 * delivered: result.n_samples = the total, n_frames the sum, hit_eos = 1 iff every segment ended on EOS, codes NULL, first_chunk_ms
 * from submit to the first document chunk. q3tts_session_cancel(id) cancels the document: from the moment it returns no further chunk
 * or SEGMENT event of the id is delivered, every running segment is retired at the next boundary, the final event is CANCELLED, and
 * the document's rows are freed. A segment that fails by itself (prompt + max_steps > n_ctx) fails the document with that status
 * (FAILED) at the boundary after; its other segments are cancelled, chunks already delivered stay delivered, other requests and
 * documents are unaffected.
 * q3tts_session_document_info (thread-safe): info[0, min(cap, *n_known)) = lo, hi, begin, end, n_frames, hit_eos, n_native, status of the
 * segments delivered so far, the values q3tts_generate_long reports (out_begin / out_end equal begin / end without a speed or rate); *n_known = how many there
 * are, *n_delivered = the samples handed out so far. This is where a subtitle track reads its times. Readable until the session closes.
 * Scheduling. Segments are internal session requests behind the prefix: they queue in the session's FIFO behind what is already there
 * and compete for slots as plain requests do; their own events are not published. Segment j is eligible iff j < head + ahead, head the
 * first segment not fully delivered: a document holds `ahead` device rows of max_steps_cap x samples per frame f32 (segment j: row j mod
 * ahead), allocated by the worker at the boundary that accepts it, checked against the free memory first (FAILED with Q3TTS_ERR_OOM, the
 * message names both numbers), freed at its end. No other boundary allocates, and submitting threads never touch the GPU. A boundary
 * with document work adds at most two launches (k_doc_scan, k_doc_emit; one more per 64 entries) and no copy: the pieces, and the
 * documents' edge tables, lie behind the plain requests' chunks in the same staging buffer. The plan of boundary t is made from the
 * lengths and edges of boundary t - 1 (whose table rode that boundary's copy): a document's chunks trail its segments by one boundary,
 * and the end of a document takes boundaries that run no frames. A document's emission is clipped to what the staging buffer has left.
 * Refusals (Q3TTS_ERR_INVALID unless stated; nothing changes): an engine-level speed or output rate is set (Q3TTS_ERR_STATE, as
 * q3tts_generate_long); join options outside their ranges; ahead outside 0..64; a break kind outside 0..4; both or neither of voice and
 * prefix; a template with a prompt; append to an unknown, closed or finished document. A document whose delivered length would pass
 * 2^28 samples fails (FAILED, Q3TTS_ERR_INVALID) at the segment that would pass it.
 * Not built: pacing by listener credit, q3tts_node_*, a per-segment voice, a per-segment speed, text_stream segments,
 * documents outside a session. Speed and output rate: below, behind q3tts_doc_opts.
 *
 * The rule. Only the head emits: the first segment not yet fully delivered. Of the head it uses n (its valid samples so far), first / last
 * (the loud-block edges of x[0, n) so far, 2.'s rule), closed (n is final) and e (the piece samples already emitted).
 *  1. trim = 1 and no loud block yet: nothing is emitted. A closed segment is then an empty piece: the head advances and the segment's
 *     kind is folded into kmax, exactly as the join does. (trim = 0: a closed segment of 0 samples is the empty piece.)
 *  2. otherwise lo = max(0, first W - keep) (trim = 0: lo = 0). lo is final from here on.
 *  3. hi_now = min(n, (last + 1) W + keep) (trim = 0: hi_now = n). It never decreases.
 *  4. an open segment emits only once hi_now - lo >= 2 fade; from then on the final F is fade. It may emit piece samples
 *     [e, hi_now - lo - fade): the final fade-out starts at or behind that point, so every emitted sample has its final value.
 *  5. a closed segment has its final hi, L and F = min(fade, L div 2). It emits [e, L), the fade-out included.
 *  6. the pause goes out directly in front of the first sample of a non-empty piece when a non-empty piece precedes it:
 *     pause_ms[kmax] * (rate / 1000) zeros; kmax is final then, because every earlier segment is closed. Never earlier: a pause is not
 *     emitted before the piece behind it is known to be non-empty.
 * When the head closes, the next segment becomes head at the same boundary: one boundary may emit the tail of a piece, several whole
 * pieces and their pauses. What a boundary emits is clipped to the room the staging buffer has left; the rest follows at the next ones.
 * Segment j may run iff j < head + ahead, and keeps its samples in document row j mod ahead. A delivered length that would pass 2^28
 * samples is Q3TTS_ERR_INVALID at the segment that would pass it. Where the chunk boundaries of a document fall is not contract; the
 * concatenation is. i16: k_pcm_pack's conversion of the f32 value, applied after the fade's multiply. */
typedef struct q3tts_doc_opts { q3tts_join_opts join; int32_t ahead /*0: 8; 1..64*/; int32_t open /*1: more segments follow*/;
    int32_t speed_permille /*0 or 1000: off; 500..2000*/; int32_t output_rate /*0 or the vocoder's rate: off; 4000..96000*/; } q3tts_doc_opts;
#define Q3TTS_EV_SEGMENT 6
/* Speed and output rate of a document (speed_permille, output_rate; both 0: everything above, launch for launch).
 * The bits. The concatenation of a document's EV_CHUNK payloads is the pcm q3tts_generate_long returns for the same template, voice,
 * segments, join options, speed_permille and output_rate — resample(time_stretch(J)), J the join — bit for bit, whatever the slot count,
 * `ahead`, the admission order, the ring sizes below and the neighbouring requests. In an i16 session the chunks are k_pcm_pack's
 * conversion of that f32 row, applied at the last stage. Chunk boundaries remain outside the contract.
 * Times. q3tts_session_document_info and EV_SEGMENT: begin / end stay in J (24 kHz); out_begin / out_end are ceil(s 1000 / speed), then
 * ceil(s L / M), exactly as q3tts_generate_long reports them. EV_SEGMENT of segment j is published at the boundary whose chunk brings the
 * delivered output count to at least out_end_j; its result.n_samples is out_end - out_begin. result.sample_rate, EV_DONE's total and
 * *n_delivered are in output samples at the output rate.
 * The pipeline. J has no row (a document may be 2^28 samples long), so up to three stages run per boundary, all in front of the
 * boundary's one device-to-host copy: (1) the plan's pieces go into a per-document f32 ring RJ that holds J at positions mod C_J (a
 * piece or pause that crosses the wrap is split in two); (2) with a speed, k_doc_tempo — k_pcm_tempo's arithmetic reading RJ mod C_J —
 * writes every decidable frame (need_k + HOLD <= |J| so far, or J is whole) into a second ring RT mod C_T; (3) with a rate,
 * k_doc_resample — k_pcm_resample's arithmetic reading RT (or RJ without a speed) — writes the decidable outputs into the staging buffer
 * behind the plain chunks and the edge tables; without a rate the stretched samples go from RT to staging as k_doc_emit pieces.
 * Flow control is host arithmetic over three counts (samples joined, frames decided, outputs delivered); nothing is read back. No stage
 * overwrites a ring position that an undecided frame or output may still read: the lower bounds are a_{k-1} + DMIN for the next
 * undecided frame k and (m M) div L - H for the next output m. The join is clipped to the free space of RJ, the stretch to that of RT,
 * the exit to the staging room; what does not fit follows at later boundaries, which run while any stage holds undelivered audio:
 * while a stage moved at the last boundary, or decidable frames or outputs are left that only a ring or the staging room held back.
 * A document's output count is bounded as its joined length is: one that would pass 2^31 - 1 output samples (speed 500 at 96 kHz can)
 * fails with Q3TTS_ERR_INVALID at the boundary that would pass it. Ring positions: J stays below 2^28, the stretched audio below 2^29.
 * An open document whose segments are all delivered keeps the held-back tail (the stretch's HOLD plus at most a hop, the resampler's
 * H) and stays silent; closing it flushes the tail in the final chunk.
 * Ring capacities are multiples of 4 and at least the span over which one frame, or one output, becomes decidable: */
#define Q3_DOC_RING_MIN_J_SPEED 1280   /* RJ under a speed: max over k, s of need_k + HOLD - (a_{k-1} + DMIN) = 256 * 2000 / 1000 + 640 + 128 */
#define Q3_DOC_RING_MIN_T_SPEED 256    /* RT without a rate: one frame (a hop) */
#define Q3_DOC_RING_MIN_RATE(H, L, M)   ((2 * (H) + 1 + ((M) + (L) - 1) / (L) + 3) & ~3)         /* the resampler's source: T = 2 H + 1 taps and one input step */
#define Q3_DOC_RING_MIN_T_RATE(H, L, M) ((2 * (H) + 1 + ((M) + (L) - 1) / (L) + 256 + 3) & ~3)   /* RT under a rate: that, and the frame that feeds it */
/* A session sizes a ring as its minimum plus what one boundary can produce (twice one slot's chunk window, stretched for RT), so a
 * boundary is not throttled by the ring: at the full shape under 100 KB for RJ and under 200 KB for RT at speed 500. The rings are
 * allocated with the document's rows (same check against the free memory, same Q3TTS_ERR_OOM message with both numbers), counted in
 * q3tts_k_device_bytes and freed with them.
 * Refusals: a speed outside {0, 1000, 500..2000} or a rate outside {0, 4000..96000} is Q3TTS_ERR_INVALID (q3tts_k_doc_rules names the
 * field); a rate pair the resampler's plan refuses is Q3TTS_ERR_UNSUPPORTED; an engine-level q3tts_set_speed / q3tts_set_output_rate
 * still refuses every document with Q3TTS_ERR_STATE: the document carries its own values, as q3tts_generate_long's opts do. */
void q3tts_doc_default_opts(q3tts_doc_opts*);
int q3tts_session_submit_document(q3tts_session* s, const q3tts_request* tmpl, const q3tts_prompt_desc* voice, q3tts_prefix* prefix,
                                  const q3tts_long_segment* segs, int32_t n_segs, const q3tts_doc_opts* opts, uint64_t* id);
int q3tts_session_document_append(q3tts_session* s, uint64_t id, const q3tts_long_segment* segs, int32_t n_segs, int32_t close);
int q3tts_session_document_info(q3tts_session* s, uint64_t id, q3tts_long_info* info, int32_t cap, int32_t* n_known, int64_t* n_delivered);
/* Test hook: from now on the worker accepts documents as if the device had at most `bytes` free (the smaller of that and what
 * hipMemGetInfo reports; < 0: off, the default), so that the Q3TTS_ERR_OOM refusal can be reached on a device that has room. A document's
 * rows are counted in q3tts_k_device_bytes from the boundary that accepts it to the one that ends it. */
int q3tts_k_session_doc_mem_cap(q3tts_session* s, int64_t bytes);
/* The rules of a well-formed document as far as no engine is needed to say them (host only): Q3TTS_ERR_STATE while an engine-level speed
 * or output rate is set (engine_speed / engine_rate != 0: a document carries its own); Q3TTS_ERR_INVALID for NULL opts, join
 * options outside their ranges, ahead outside 0..64, speed_permille outside {0, 500..2000}, output_rate outside {0, 4000..96000},
 * open outside 0 / 1, n_segs outside 1..1024 (0 allowed with open = 1), a break kind
 * outside 0..4, both or neither of voice and prefix. msg receives the rule, at most cap - 1 characters (may be NULL). */
int q3tts_k_doc_rules(const q3tts_doc_opts* opts, const int32_t* kinds, int32_t n_segs, int32_t have_voice, int32_t have_prefix,
                      int32_t engine_speed, int32_t engine_rate, char* msg, int32_t cap);
/* One boundary of the host plan (host only). segs [n_segs][5] = n, first, last, closed, kind of every segment as of this boundary
 * ({INT32_MAX, -1}: no loud block); room: the samples the staging buffer has left; state [7], all zero before the first call, carries the
 * document between calls (state[0] = head, state[5] = samples delivered). pieces [cap][6] = seg (-1: a run of zeros), the first sample's
 * offset in the segment's row, its index j0 in the piece, count, the piece's final length L (-1: the segment is open), F; done
 * [done_cap][5] = seg, lo, hi, begin, end of every segment whose piece (possibly empty) this call has handed out completely — the values
 * q3tts_generate_long reports. *n_pieces / *n_done are set even when a capacity is too small (then Q3TTS_ERR_INVALID). */
int q3tts_k_doc_plan(const q3tts_join_opts* opts, int32_t rate, const int32_t* segs, int32_t n_segs, int64_t room, int64_t* state,
                     int64_t* pieces, int32_t cap, int32_t* n_pieces, int64_t* done, int32_t done_cap, int32_t* n_done);
/* scan + plan + emit, boundary by boundary, as a session would drive them. src [rows][stride] f32 are the segments' PCM rows, uploaded as
 * they are (the tests put NaN behind every valid length). sched [rows][sched_stride]: segment i's valid length after each boundary at
 * which it runs, ascending, sched_n[i] >= 1 entries, the last one final. At a boundary every segment j in [head, head + ahead) that is
 * not closed takes its next length: one k_doc_scan launch copies the new samples into document row j mod ahead and updates the edges.
 * The plan is made from this boundary's lengths and edges (lag = 0) or from the previous boundary's (lag = 1, the session's form: the
 * edges ride the copy of the boundary before), with room = staging - dst0; one k_doc_emit launch per 64 pieces writes the pieces into a
 * staging buffer of `staging` samples (format 0: f32, 1: i16) at dst0, behind where the plain requests' chunks would lie. out receives
 * the concatenation (*n_out samples), chunks[b] the samples of boundary b (*n_bounds of them, at most chunk_cap), plan [rows][4] = lo, hi,
 * begin, end. *bad counts what must not happen: a staging byte outside [dst0, dst0 + chunk) that lost its uploaded value, and with
 * check_rows != 0 any element of the document rows that differs from "the samples copied so far, the uploaded fill elsewhere". */
int q3tts_k_doc_stream(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* kinds, const int32_t* sched,
                       const int32_t* sched_n, int32_t sched_stride, const q3tts_join_opts* opts, int32_t rate, int32_t ahead, int32_t lag,
                       int64_t staging, int64_t dst0, int32_t format, int32_t check_rows, void* out, int64_t out_cap, int64_t* n_out,
                       int64_t* chunks, int32_t chunk_cap, int32_t* n_bounds, int64_t* plan, int64_t* bad);
/* The same with a speed and / or an output rate (at least one): scan -> plan -> join into RJ -> stretch into RT -> exit, boundary by
 * boundary, on uploaded rows; `rate` is the rows' rate and the resampler's input rate. ring_j / ring_t: the rings' capacities (0: the
 * minimum; below the minimum or no multiple of 4: Q3TTS_ERR_INVALID). `staging` and chunks[b] are in OUTPUT samples. A segment whose
 * schedule repeats its last length stays open at that length until the schedule's last entry (a segment closed late). delta
 * [delta_cap] receives delta_k of every frame (*n_frames of them; NULL with delta_cap = 0). *bad counts every staging byte outside
 * the emitted range that lost its fill. That no ring element was overwritten while a later read still needed it is checked by the final
 * equality, not by a shadow of J: the tests compare out with the one-shot composition over rings at their minimum. */
int q3tts_k_doc_stream_rate(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* kinds, const int32_t* sched,
                            const int32_t* sched_n, int32_t sched_stride, const q3tts_join_opts* opts, int32_t rate, int32_t ahead, int32_t lag,
                            int64_t staging, int64_t dst0, int32_t format, int32_t check_rows, void* out, int64_t out_cap, int64_t* n_out,
                            int64_t* chunks, int32_t chunk_cap, int32_t* n_bounds, int64_t* plan, int64_t* bad, int32_t speed_permille,
                            int32_t output_rate, int64_t ring_j, int64_t ring_t, int32_t* delta, int32_t delta_cap, int32_t* n_frames);
/* One boundary of the pipeline's flow control (host only). state [4] = samples joined, J whole, frames decided, outputs delivered (all
 * zero before the first call; updated). The join has `want` more samples to hand out (fin_if_all: J is whole once all of them are);
 * room_out: the staging room in output samples; ring_j / ring_t as above. out [13] = the join's room, samples joined, k_from, k_to,
 * stretched samples after them, the exit's valid source samples, whether those are all, the first output, the count, whether the
 * document is now wholly delivered, the two minimum capacities, and `pending`: decidable frames or outputs are left that only the
 * free space of RT or room_out held back — the worker must not sleep then, whether or not anything moved at this boundary. */
int q3tts_k_doc_ring_plan(int32_t speed_permille, int32_t rate_in, int32_t rate_out, int64_t ring_j, int64_t ring_t, int64_t* state,
                          int64_t want, int32_t fin_if_all, int64_t room_out, int64_t* out);
/* out_begin / out_end as the session computes them (host only): *out = position pos of J through ceil(s 1000 / speed), then ceil(s L / M) */
int q3tts_k_doc_out_pos(int64_t pos, int32_t speed_permille, int32_t rate_in, int32_t rate_out, int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* Q3TTS_H */
