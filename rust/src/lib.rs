//! `extern "C"` declarations of include/q3tts.h and a safe wrapper that keeps the reference crate's names:
//! `TtsEngine::{new, set_max_steps, set_sampler_config, generate_with_voice}`, `SamplerConfig`, `VoiceFile`,
//! `AudioSample`. UNCOMPILED (no Rust toolchain in the image); field order mirrors the C header one to one.
#![allow(non_camel_case_types)]
use std::ffi::CStr;
use std::os::raw::{c_char, c_float, c_int};

#[repr(C)] #[derive(Clone, Copy)]
pub struct q3tts_model_config {
    pub t_n_layer: i32, pub t_d_model: i32, pub t_n_head: i32, pub t_n_kv_head: i32, pub t_head_dim: i32, pub t_d_ffn: i32, pub t_vocab: i32,
    pub t_rope_theta: c_float, pub t_mrope_sections: [i32; 4],
    pub p_n_layer: i32, pub p_d_model: i32, pub p_n_head: i32, pub p_n_kv_head: i32, pub p_head_dim: i32, pub p_d_ffn: i32,
    pub p_rope_theta: c_float, pub n_codebooks: i32, pub codebook_size: i32, pub rms_eps: c_float,
    pub d_embed: i32, pub text_vocab: i32, pub codec0_rows: i32, pub codecq_rows: i32,
    pub sample_limit: i32, pub eos_code: i32, pub tts_pad_id: i32,
}
#[repr(C)] #[derive(Clone, Copy)]
pub struct q3tts_vocoder_config {
    pub n_codebooks: i32, pub codebook_size: i32, pub codebook_dim: i32, pub latent_dim: i32, pub pre_conv_kernel: i32,
    pub n_layer: i32, pub n_head: i32, pub head_dim: i32, pub d_ffn: i32, pub sliding_window: i32,
    pub rope_theta: c_float, pub rms_eps: c_float, pub layer_scale_init: c_float,
    pub n_upsample: i32, pub upsample_ratios: [i32; 4], pub decoder_dim: i32, pub n_dec_blocks: i32, pub dec_rates: [i32; 8],
    pub lookahead_frames: i32, pub sample_rate: i32,
}
#[repr(C)]
pub struct q3tts_engine_config {
    pub model: q3tts_model_config, pub vocoder: q3tts_vocoder_config,
    pub device: i32, pub max_batch: i32, pub n_ctx: i32, pub max_steps_cap: i32, pub with_vocoder: i32,
    pub synth_seed: u64, pub weights_path: *const c_char,
    pub talker_q8_0: i32,   // 2: the Talker's Q8_0 blocks stay quantised on the device and meet Q8_0 activations (W8A8, the crate's default "q8_0" directory); 1: W8A16; 0: bf16
    pub vocoder_flush_tail: i32,   // 0: the look-ahead tail is flushed as the reference does (only when n_frames % 4 != 0); 1: always
    pub predictor_q8_0: i32,   // 0: bf16 Predictor; 2: its Q8_0 blocks stay quantised on the device and meet Q8_0 activations (W8A8), opt-in; 1: refused
    pub kv_q8_0: i32,   // 0: bf16 Talker K/V cache; 1: the cache as ggml Q8_0 blocks on the device (0.53 of the bytes; results differ from the bf16 cache's), opt-in; else refused
}
#[repr(C)]
pub struct q3tts_prompt_desc {
    pub text_ids: *const u32, pub n_text: i32, pub instruct_ids: *const u32, pub n_instruct: i32,
    pub lang_id: i32, pub spk_id: i32, pub spk_emb: *const c_float,
    pub ref_codes: *const i32, pub n_ref_frames: i32, pub ref_text_ids: *const u32, pub n_ref_text: i32,
}
#[repr(C)]
pub struct q3tts_request {
    pub prompt_embd: *const c_float, pub n_tok: i32,
    pub text_stream: i32,   // 1: the streamed text layout (include/q3tts.h, "streaming text input"); 0: the whole text is in the prompt. In the gap behind n_tok
    pub prompt: *const q3tts_prompt_desc, pub use_engine_sampler: i32,
    pub temperature: c_float, pub top_k: i32, pub top_p: c_float, pub has_seed: i32,
    pub text_open: i32,     // sessions only: 1 = more text follows (q3tts_session_append_text); 0: the text is closed. In the gap behind has_seed
    pub seed: u64,
    pub max_steps: i32, pub min_frames: i32, pub force_eos_at: i32, pub want_pcm: i32,
    pub prefix: *const q3tts_prefix,   // null, or a voice prefix of the same engine: the prompt is its rows followed by this request's own
}
#[repr(C)]
pub struct q3tts_result {
    pub status: i32, pub n_frames: i32, pub hit_eos: i32, pub codes: *mut i32, pub pcm: *mut c_float,
    pub n_samples: i32, pub sample_rate: i32, pub first_chunk_ms: c_float, pub total_ms: c_float,
}
pub enum q3tts_engine {}
pub enum q3tts_stream {}
pub enum q3tts_node {}
pub enum q3tts_prefix {}
pub enum q3tts_session {}
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct q3tts_node_timings { pub generate_ms: c_float, pub gather_ms: c_float, pub total_ms: c_float, pub gathered_bytes: i64, pub n_devices: i32 }

// long documents (include/q3tts.h, "long documents"): the splitter's spans, the join's options, a document's segments and its result
pub const Q3TTS_BREAK_END: i32 = 0;
pub const Q3TTS_BREAK_HARD: i32 = 1;
pub const Q3TTS_BREAK_CLAUSE: i32 = 2;
pub const Q3TTS_BREAK_SENTENCE: i32 = 3;
pub const Q3TTS_BREAK_PARAGRAPH: i32 = 4;
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct q3tts_text_span { pub begin: i64, pub end: i64, pub kind: i32 }
#[repr(C)] #[derive(Clone, Copy)]
pub struct q3tts_join_opts { pub trim: i32, pub threshold: c_float, pub keep: i32, pub fade: i32, pub pause_ms: [i32; 5] }
#[repr(C)]
pub struct q3tts_long_segment { pub ids: *const u32, pub n_ids: i32, pub kind: i32, pub max_steps: i32 }
/// q3tts_session_event.kind of a document's segment whose piece has gone out (include/q3tts.h, "documents in a session")
pub const Q3TTS_EV_SEGMENT: i32 = 6;
#[repr(C)] #[derive(Clone, Copy)]
pub struct q3tts_doc_opts { pub join: q3tts_join_opts, pub ahead: i32, pub open: i32, pub speed_permille: i32, pub output_rate: i32 }
#[repr(C)] #[derive(Clone, Copy)]
pub struct q3tts_long_opts { pub join: q3tts_join_opts, pub speed_permille: i32, pub output_rate: i32 }
#[repr(C)] #[derive(Clone, Copy)]
pub struct q3tts_long_info {
    pub status: i32, pub n_frames: i32, pub hit_eos: i32, pub n_native: i64, pub lo: i64, pub hi: i64,
    pub begin: i64, pub end: i64, pub out_begin: i64, pub out_end: i64,
}
#[repr(C)]
pub struct q3tts_long_result {
    pub status: i32, pub n_segments: i32, pub n_truncated: i32, pub sample_rate: i32, pub n_samples: i64, pub pcm: *mut c_float,
    pub info: *mut q3tts_long_info, pub generate_ms: c_float, pub join_ms: c_float, pub total_ms: c_float,
}

#[link(name = "q3tts")]
extern "C" {
    // long documents (no counterpart in the reference, whose generate_with_voice truncates one text at 512 steps): split on the host,
    // the segments as one batch behind a voice prefix, their PCM trimmed, faded and joined on the device, one copy to the host
    pub fn q3tts_text_split(utf8: *const c_char, n_bytes: i64, target_bytes: i32, max_bytes: i32, spans: *mut q3tts_text_span, cap: i32,
                            n_spans: *mut i32, err: *mut c_char, err_cap: i32) -> c_int;
    pub fn q3tts_long_default_opts(o: *mut q3tts_long_opts);
    pub fn q3tts_generate_long(e: *mut q3tts_engine, tmpl: *const q3tts_request, voice: *const q3tts_prompt_desc, prefix: *const q3tts_prefix,
                               segs: *const q3tts_long_segment, n_segs: i32, opts: *const q3tts_long_opts, out: *mut q3tts_long_result) -> c_int;
    pub fn q3tts_long_result_free(r: *mut q3tts_long_result);
    pub fn q3tts_pcm_join(e: *mut q3tts_engine, clips: *const *const c_float, n: *const i64, kinds: *const i32, n_clips: i32,
                          opts: *const q3tts_join_opts, out: *mut c_float, cap: i64, n_out: *mut i64, edges: *mut i64) -> c_int;
    pub fn q3tts_default_config(cfg: *mut q3tts_engine_config);
    // every model dimension and weights_path from the files of model_dir's quant directory (host only); errors go to err, cfg is then unchanged
    pub fn q3tts_config_from_model_dir(model_dir: *const c_char, quant: *const c_char, cfg: *mut q3tts_engine_config, path_buf: *mut c_char, path_cap: i32,
                                       err: *mut c_char, err_cap: i32) -> c_int;
    pub fn q3tts_engine_create(cfg: *const q3tts_engine_config, out: *mut *mut q3tts_engine) -> c_int;
    pub fn q3tts_engine_destroy(e: *mut q3tts_engine);
    // where the vocoder's weights came from: 0 none, 1 seeded synthetic, 2 qwen3_tts_vocoder.gguf beside the model
    pub fn q3tts_get_vocoder_source(e: *const q3tts_engine, source: *mut i32) -> c_int;
    pub fn q3tts_last_error(e: *const q3tts_engine) -> *const c_char;
    pub fn q3tts_set_sampler(e: *mut q3tts_engine, temperature: c_float, top_k: i32, top_p: c_float, has_seed: i32, seed: u64) -> c_int;
    pub fn q3tts_set_max_steps(e: *mut q3tts_engine, max_steps: i32) -> c_int;
    // Predictor sampler and code-0 repetition penalty: engine state, no counterpart in the reference (greedy Predictor, no penalty)
    pub fn q3tts_set_predictor_sampler(e: *mut q3tts_engine, temperature: c_float, top_k: i32, top_p: c_float) -> c_int;
    pub fn q3tts_get_predictor_sampler(e: *const q3tts_engine, temperature: *mut c_float, top_k: *mut i32, top_p: *mut c_float) -> c_int;
    pub fn q3tts_set_repetition_penalty(e: *mut q3tts_engine, penalty: c_float) -> c_int;
    pub fn q3tts_get_repetition_penalty(e: *const q3tts_engine, penalty: *mut c_float) -> c_int;
    pub fn q3tts_generate(e: *mut q3tts_engine, req: *const q3tts_request, out: *mut q3tts_result) -> c_int;
    pub fn q3tts_generate_batch(e: *mut q3tts_engine, reqs: *const q3tts_request, n: i32, outs: *mut q3tts_result) -> c_int;
    pub fn q3tts_result_free(r: *mut q3tts_result);
    // streaming: 4-frame (64-code) chunks as the reference's vocoder thread produces them (src/tts/engine.rs:507-541)
    pub fn q3tts_stream_begin(e: *mut q3tts_engine, req: *const q3tts_request, out: *mut *mut q3tts_stream) -> c_int;
    pub fn q3tts_stream_poll(s: *mut q3tts_stream, chunk: *mut *const c_float, n_samples: *mut i32, is_final: *mut i32) -> c_int;
    pub fn q3tts_stream_end(s: *mut q3tts_stream, out_codes_optional: *mut q3tts_result) -> c_int;
    pub fn q3tts_free(p: *mut std::ffi::c_void);
    // voice prefixes (no counterpart in the reference, which rebuilds the whole prompt per call): the Talker's K/V of a voice part, kept on
    // the device; exactly one of p (n_text == 0) or embd / n_tok is given
    pub fn q3tts_prefix_create(e: *mut q3tts_engine, p: *const q3tts_prompt_desc, embd: *const c_float, n_tok: i32, out: *mut *mut q3tts_prefix) -> c_int;
    pub fn q3tts_prefix_rows(x: *const q3tts_prefix) -> i32;
    pub fn q3tts_prefix_destroy(x: *mut q3tts_prefix) -> c_int;
    // paced requests and swapping (include/q3tts.h; sessions are otherwise driven through the C header): a frame credit per request,
    // granted as the listener plays, and a device arena that parked requests are swapped out into while others wait for their slots
    pub fn q3tts_session_submit_paced(s: *mut q3tts_session, req: *const q3tts_request, credit_frames: i32, id: *mut u64) -> c_int;
    pub fn q3tts_session_grant(s: *mut q3tts_session, id: u64, frames: i32) -> c_int;
    // documents in a session (include/q3tts.h): a long document streams in order while later segments run; the chunks of its id, joined,
    // are q3tts_generate_long's pcm bit for bit. Q3TTS_EV_SEGMENT (6) reports each segment as its piece has gone out
    pub fn q3tts_k_session_doc_mem_cap(s: *mut q3tts_session, bytes: i64) -> c_int;
    pub fn q3tts_doc_default_opts(o: *mut q3tts_doc_opts);
    pub fn q3tts_session_submit_document(s: *mut q3tts_session, tmpl: *const q3tts_request, voice: *const q3tts_prompt_desc, prefix: *mut q3tts_prefix,
                                         segs: *const q3tts_long_segment, n_segs: i32, opts: *const q3tts_doc_opts, id: *mut u64) -> c_int;
    pub fn q3tts_session_document_append(s: *mut q3tts_session, id: u64, segs: *const q3tts_long_segment, n_segs: i32, close: i32) -> c_int;
    pub fn q3tts_session_document_info(s: *mut q3tts_session, id: u64, info: *mut q3tts_long_info, cap: i32, n_known: *mut i32, n_delivered: *mut i64) -> c_int;
    pub fn q3tts_session_set_swap(s: *mut q3tts_session, arena_bytes: i64) -> c_int;
    pub fn q3tts_session_swap_stats(s: *const q3tts_session, out: *mut i64) -> c_int;
    // speaking rate (no counterpart in the reference): engine state in per mille, 500..2000, 0 or 1000 = off; a pitch-preserving time-stretch on the device
    pub fn q3tts_set_speed(e: *mut q3tts_engine, permille: i32) -> c_int;
    pub fn q3tts_get_speed(e: *const q3tts_engine, permille: *mut i32) -> c_int;
    // output sample rate (no counterpart in the reference, which emits 24 kHz only): engine state, 4000..96000 Hz, 0 or 24000 = off
    pub fn q3tts_set_output_rate(e: *mut q3tts_engine, rate: i32) -> c_int;
    pub fn q3tts_get_output_rate(e: *const q3tts_engine, rate: *mut i32) -> c_int;
    // one node, several GPUs (no counterpart in the reference: n_seq_max = 1, src/models/llama/mod.rs:413): one engine + host thread per device
    // inside the library, request i on device i % n_devices, optional RCCL gather of the i16 PCM to the first device
    pub fn q3tts_node_create(cfg: *const q3tts_engine_config, devices: *const i32, n_devices: i32, out: *mut *mut q3tts_node) -> c_int;
    pub fn q3tts_node_destroy(n: *mut q3tts_node);
    pub fn q3tts_node_generate_batch(n: *mut q3tts_node, reqs: *const q3tts_request, n_reqs: i32, outs: *mut q3tts_result, pcm_i16: *mut *mut i16) -> c_int;
    pub fn q3tts_node_get_timings(n: *const q3tts_node, out: *mut q3tts_node_timings) -> c_int;
    pub fn q3tts_node_last_error(n: *const q3tts_node) -> *const c_char;
    // voice-clone encoders (replace AudioEncoder / SpeakerEncoder, src/models/onnx.rs:82-160)
    pub fn q3tts_clone_default_config(cfg: *mut q3tts_clone_config);
    pub fn q3tts_clone_init(e: *mut q3tts_engine, cfg: *const q3tts_clone_config) -> c_int;
    // trained encoder weights from qwen3_tts_speaker_encoder.gguf / qwen3_tts_codec_encoder.gguf, found in weights_dir or its parent
    // (NULL: the engine's own weights_path); host-only shape query, loader, source (0 not loaded, 1 synthetic, 2 files), host-only test hook
    pub fn q3tts_clone_config_from_dir(weights_dir: *const c_char, cfg: *mut q3tts_clone_config, err: *mut c_char, err_cap: i32) -> c_int;
    pub fn q3tts_clone_load(e: *mut q3tts_engine, weights_dir: *const c_char) -> c_int;
    pub fn q3tts_get_clone_source(e: *const q3tts_engine, source: *mut i32) -> c_int;
    // where the two files are (each path into its buffer of cap bytes, "" when absent): returns how many were found, or a negative status
    pub fn q3tts_clone_files_find(weights_dir: *const c_char, speaker_path: *mut c_char, codec_path: *mut c_char, cap: i32) -> c_int;
    // host-only test hook: the host half of q3tts_clone_load (open, shape, cross-checks, finite values, config rules) with its status
    pub fn q3tts_k_clone_load_check(weights_dir: *const c_char) -> c_int;
    pub fn q3tts_k_clone_file_tensor(weights_dir: *const c_char, cfg: *const q3tts_clone_config, comp: i32, which: i32, out: *mut c_float, cap: i64,
                                     n: *mut i64) -> c_int;
    pub fn q3tts_clone_audio_frames(e: *const q3tts_engine, n_samples: i64) -> i32;
    pub fn q3tts_clone_audio_encode(e: *mut q3tts_engine, audio: *const c_float, n_samples: i64, codes: *mut i64, cap_frames: i32, n_frames: *mut i32) -> c_int;
    pub fn q3tts_clone_speaker_encode(e: *mut q3tts_engine, audio: *const c_float, n_samples: i64, spk_emb: *mut c_float) -> c_int;
}

/// q3tts_clone_config (include/q3tts.h), field for field
#[repr(C)]
#[derive(Clone, Copy)]
pub struct q3tts_clone_config {
    pub mel_dim: i32,
    pub se_channels: [i32; 5], pub se_kernels: [i32; 5], pub se_dilations: [i32; 5],
    pub se_attn_channels: i32, pub se_res2net_scale: i32, pub se_se_channels: i32, pub se_dim: i32,
    pub ae_filters: i32, pub ae_kernel: i32, pub ae_res_kernel: i32, pub ae_last_kernel: i32,
    pub ae_n_ratios: i32, pub ae_ratios: [i32; 4],
    pub ae_hidden: i32, pub ae_n_layer: i32, pub ae_n_head: i32, pub ae_head_dim: i32, pub ae_d_ffn: i32, pub ae_window: i32,
    pub ae_rope_theta: c_float, pub ae_ln_eps: c_float, pub ae_layer_scale: c_float,
    pub ae_down_stride: i32, pub ae_vq_dim: i32, pub ae_n_codebooks: i32, pub ae_codebook_size: i32,
}

// ---- the reference crate's public names on top of the C ABI (src/lib.rs:11-20) ------------------------------------
#[derive(Debug, Clone)]
pub struct SamplerConfig { pub temperature: f32, pub top_k: i32, pub top_p: f32, pub seed: Option<u64> }
impl Default for SamplerConfig { fn default() -> Self { Self { temperature: 0.7, top_k: 40, top_p: 0.9, seed: None } } }

pub struct VoiceFile { pub ref_text: String, pub audio_codes: Vec<i64>, pub speaker_embedding: Vec<f32> }
pub struct AudioSample { pub samples: Vec<f32>, pub sample_rate: u32, pub channels: u16 }

pub struct TtsEngine { raw: *mut q3tts_engine, sampler: SamplerConfig, max_steps: usize }

impl TtsEngine {
    /// TtsEngine::new(model_dir, quant) — src/tts/engine.rs:84-169. `model_dir/<quant dir>` (src/tts/engine.rs:91-95) holds
    /// qwen3_tts_talker.gguf, qwen3_tts_predictor.gguf and qwen3_assets.gguf (or the NPY assets). Every model dimension comes from those
    /// files (q3tts_config_from_model_dir), as llama.cpp reads them for the reference: no shape is assumed here. The same call takes the
    /// vocoder's shape from qwen3_tts_vocoder.gguf when that file lies in the quant directory or in `model_dir`; the engine then loads it.
    pub fn new(model_dir: &str, quant: &str) -> Result<Self, String> {
        let dir = std::ffi::CString::new(model_dir).map_err(|e| e.to_string())?;
        let q = std::ffi::CString::new(quant).map_err(|e| e.to_string())?;
        let mut path_buf: Vec<c_char> = vec![0; model_dir.len() + 16];   // model_dir + '/' + the longest quant directory name + NUL
        let mut err: Vec<c_char> = vec![0; 1024];
        unsafe {
            let mut cfg: q3tts_engine_config = std::mem::zeroed();
            q3tts_default_config(&mut cfg);
            let rc = q3tts_config_from_model_dir(dir.as_ptr(), q.as_ptr(), &mut cfg, path_buf.as_mut_ptr(), path_buf.len() as i32,
                                                 err.as_mut_ptr(), err.len() as i32);
            if rc != 0 { return Err(format!("q3tts_config_from_model_dir failed ({}): {}", rc, CStr::from_ptr(err.as_ptr()).to_string_lossy())); }
            // cfg.weights_path now points into path_buf: borrowed for the call only
            cfg.talker_q8_0 = if quant == "q8_0" { 2 } else { 0 };   // gguf_q8_0: the Talker's blocks stay as stored and are multiplied as llama.cpp does (Q8_0 x Q8_0, W8A8)
            let mut raw = std::ptr::null_mut();
            let rc = q3tts_engine_create(&cfg, &mut raw);
            if rc != 0 { return Err(format!("q3tts_engine_create failed ({}): {}", rc, CStr::from_ptr(q3tts_last_error(std::ptr::null())).to_string_lossy())); }
            Ok(Self { raw, sampler: SamplerConfig::default(), max_steps: 512 })
        }
    }
    /// true: the vocoder runs on seeded synthetic weights (no qwen3_tts_vocoder.gguf was found), so the PCM is not speech
    pub fn vocoder_is_synthetic(&self) -> Result<bool, String> {
        let mut src = 0i32;
        let rc = unsafe { q3tts_get_vocoder_source(self.raw, &mut src) };
        self.check(rc, "q3tts_get_vocoder_source")?;
        Ok(src == 1)
    }
    /// where the clone encoders' weights came from: 0 not loaded, 1 seeded synthetic (q3tts_clone_init), 2 the two encoder files (q3tts_clone_load)
    pub fn clone_source(&self) -> Result<i32, String> {
        let mut src = 0i32;
        let rc = unsafe { q3tts_get_clone_source(self.raw, &mut src) };
        self.check(rc, "q3tts_get_clone_source")?;
        Ok(src)
    }
    pub fn set_max_steps(&mut self, steps: usize) { self.max_steps = steps; }
    pub fn set_sampler_config(&mut self, c: SamplerConfig) { self.sampler = c; }
    pub fn get_sampler_config(&self) -> &SamplerConfig { &self.sampler }
    fn check(&self, rc: c_int, what: &str) -> Result<(), String> {
        if rc == 0 { Ok(()) } else { Err(format!("{} failed ({}): {}", what, rc, unsafe { CStr::from_ptr(q3tts_last_error(self.raw)) }.to_string_lossy())) }
    }
    /// Sampler of the 15 residual codes of every frame for requests admitted from now on (temperature 0 = greedy, the default; the
    /// reference's Predictor is always greedy). `c.seed` is ignored: the Predictor's draws derive from each request's own seed.
    pub fn set_predictor_sampler_config(&mut self, c: &SamplerConfig) -> Result<(), String> {
        let rc = unsafe { q3tts_set_predictor_sampler(self.raw, c.temperature, c.top_k, c.top_p) };
        self.check(rc, "q3tts_set_predictor_sampler")
    }
    pub fn get_predictor_sampler_config(&self) -> Result<SamplerConfig, String> {
        let (mut t, mut k, mut p) = (0.0 as c_float, 0i32, 0.0 as c_float);
        let rc = unsafe { q3tts_get_predictor_sampler(self.raw, &mut t, &mut k, &mut p) };
        self.check(rc, "q3tts_get_predictor_sampler")?;
        Ok(SamplerConfig { temperature: t, top_k: k, top_p: p, seed: None })
    }
    /// Repetition penalty on the Talker's code-0 logits over the codes generated so far; 1.0 = off (the default).
    pub fn set_repetition_penalty(&mut self, p: f32) -> Result<(), String> {
        let rc = unsafe { q3tts_set_repetition_penalty(self.raw, p) };
        self.check(rc, "q3tts_set_repetition_penalty")
    }
    pub fn get_repetition_penalty(&self) -> Result<f32, String> {
        let mut p = 0.0 as c_float;
        let rc = unsafe { q3tts_get_repetition_penalty(self.raw, &mut p) };
        self.check(rc, "q3tts_get_repetition_penalty")?;
        Ok(p)
    }

    /// generate_with_voice — src/tts/engine.rs:390. `text_ids` = tokenizer.encode(text) (the tokenizer stays in Rust).
    pub fn generate_with_voice(&mut self, text_ids: &[u32], voice: &VoiceFile, instruct_ids: Option<&[u32]>) -> Result<AudioSample, String> {
        let codes32: Vec<i32> = voice.audio_codes.iter().map(|&c| c as i32).collect();
        let desc = q3tts_prompt_desc {
            text_ids: text_ids.as_ptr(), n_text: text_ids.len() as i32,
            instruct_ids: instruct_ids.map_or(std::ptr::null(), |s| s.as_ptr()), n_instruct: instruct_ids.map_or(0, |s| s.len() as i32),
            lang_id: 2055, spk_id: -1, spk_emb: voice.speaker_embedding.as_ptr(),
            ref_codes: if codes32.is_empty() { std::ptr::null() } else { codes32.as_ptr() }, n_ref_frames: (codes32.len() / 16) as i32,
            ref_text_ids: std::ptr::null(), n_ref_text: 0, // tokenizer.encode(&voice.ref_text) in the real crate
        };
        let req = q3tts_request {
            prompt_embd: std::ptr::null(), n_tok: 0, prompt: &desc, use_engine_sampler: 0,
            temperature: self.sampler.temperature, top_k: self.sampler.top_k, top_p: self.sampler.top_p,
            has_seed: self.sampler.seed.is_some() as i32, seed: self.sampler.seed.unwrap_or(0),
            max_steps: self.max_steps as i32, min_frames: 0, force_eos_at: -1, want_pcm: 1, prefix: std::ptr::null(), text_stream: 0, text_open: 0,
        };
        unsafe {
            let mut out: q3tts_result = std::mem::zeroed();
            let rc = q3tts_generate(self.raw, &req, &mut out);
            if rc != 0 { return Err(CStr::from_ptr(q3tts_last_error(self.raw)).to_string_lossy().into_owned()); }
            let samples = std::slice::from_raw_parts(out.pcm, out.n_samples as usize).to_vec();
            q3tts_result_free(&mut out);
            Ok(AudioSample { samples, sample_rate: 24000, channels: 1 })
        }
    }
}
/// One segment of a document: its text, where it lies in the audio (seconds) and whether it ended by EOS (false: it ran into max_steps).
pub struct LongSegment { pub text: String, pub t_begin_s: f64, pub t_end_s: f64, pub hit_eos: bool }

impl TtsEngine {
    /// A document of any length in one voice (no counterpart in the reference; include/q3tts.h, "long documents"): the text is split by
    /// q3tts_text_split, every span is encoded on its own by `encode` (the tokenizer stays in Rust) and runs as a segment of one batch behind
    /// a prefix made from the voice; the segments' PCM is trimmed, faded and joined on the device and copied to the host once.
    /// `speed`: Some(1.25) = a quarter faster, the pitch kept; `sample_rate`: Some(16000), ...; None = off / the vocoder's 24 kHz.
    pub fn generate_long(&mut self, text: &str, voice: &VoiceFile, instruct_ids: Option<&[u32]>, encode: &dyn Fn(&str) -> Vec<u32>,
                         speed: Option<f32>, sample_rate: Option<u32>) -> Result<(AudioSample, Vec<LongSegment>), String> {
        let mut err: Vec<c_char> = vec![0; 256];
        let mut spans = vec![q3tts_text_span::default(); 64];
        let mut n = 0i32;
        unsafe {
            let mut rc = q3tts_text_split(text.as_ptr() as *const c_char, text.len() as i64, 0, 0, spans.as_mut_ptr(), spans.len() as i32, &mut n,
                                          err.as_mut_ptr(), err.len() as i32);
            if rc != 0 && n as usize > spans.len() {   // *n_spans carries the size needed
                spans.resize(n as usize, q3tts_text_span::default());
                rc = q3tts_text_split(text.as_ptr() as *const c_char, text.len() as i64, 0, 0, spans.as_mut_ptr(), spans.len() as i32, &mut n,
                                      err.as_mut_ptr(), err.len() as i32);
            }
            if rc != 0 { return Err(format!("q3tts_text_split failed ({}): {}", rc, CStr::from_ptr(err.as_ptr()).to_string_lossy())); }
        }
        spans.truncate(n as usize);
        if spans.is_empty() { return Err("generate_long: the text holds nothing speakable".into()); }
        let pieces: Vec<&str> = spans.iter().map(|s| &text[s.begin as usize..s.end as usize]).collect();
        let ids: Vec<Vec<u32>> = pieces.iter().map(|p| encode(p)).collect();
        let segs: Vec<q3tts_long_segment> = ids.iter().zip(spans.iter())
            .map(|(v, s)| q3tts_long_segment { ids: v.as_ptr(), n_ids: v.len() as i32, kind: s.kind, max_steps: 0 }).collect();
        let codes32: Vec<i32> = voice.audio_codes.iter().map(|&c| c as i32).collect();
        let vdesc = q3tts_prompt_desc {
            text_ids: std::ptr::null(), n_text: 0,
            instruct_ids: instruct_ids.map_or(std::ptr::null(), |s| s.as_ptr()), n_instruct: instruct_ids.map_or(0, |s| s.len() as i32),
            lang_id: 2055, spk_id: -1, spk_emb: voice.speaker_embedding.as_ptr(),
            ref_codes: if codes32.is_empty() { std::ptr::null() } else { codes32.as_ptr() }, n_ref_frames: (codes32.len() / 16) as i32,
            ref_text_ids: std::ptr::null(), n_ref_text: 0,
        };
        let tmpl = q3tts_request {
            prompt_embd: std::ptr::null(), n_tok: 0, prompt: std::ptr::null(), use_engine_sampler: 0,
            temperature: self.sampler.temperature, top_k: self.sampler.top_k, top_p: self.sampler.top_p,
            has_seed: self.sampler.seed.is_some() as i32, seed: self.sampler.seed.unwrap_or(0),
            max_steps: self.max_steps as i32, min_frames: 0, force_eos_at: -1, want_pcm: 0, prefix: std::ptr::null(), text_stream: 0, text_open: 0,
        };
        unsafe {
            let (mut eng_speed, mut eng_rate) = (0i32, 0i32);   // the engine's own speed and rate are for plain requests: cleared around the call
            q3tts_get_speed(self.raw, &mut eng_speed);
            q3tts_get_output_rate(self.raw, &mut eng_rate);
            let mut opts: q3tts_long_opts = std::mem::zeroed();
            q3tts_long_default_opts(&mut opts);
            opts.speed_permille = speed.map_or(eng_speed, |s| (s * 1000.0).round() as i32);
            opts.output_rate = sample_rate.map_or(eng_rate, |r| r as i32);
            q3tts_set_speed(self.raw, 0);
            q3tts_set_output_rate(self.raw, 0);
            let mut out: q3tts_long_result = std::mem::zeroed();
            let rc = q3tts_generate_long(self.raw, &tmpl, &vdesc, std::ptr::null(), segs.as_ptr(), segs.len() as i32, &opts, &mut out);
            let msg = if rc != 0 { CStr::from_ptr(q3tts_last_error(self.raw)).to_string_lossy().into_owned() } else { String::new() };
            q3tts_set_output_rate(self.raw, eng_rate);
            q3tts_set_speed(self.raw, eng_speed);
            if rc != 0 { q3tts_long_result_free(&mut out); return Err(msg); }
            let samples = std::slice::from_raw_parts(out.pcm, out.n_samples as usize).to_vec();
            let r = out.sample_rate as f64;
            let info = std::slice::from_raw_parts(out.info, out.n_segments as usize);
            let table = pieces.iter().zip(info.iter()).map(|(p, f)| LongSegment {
                text: p.to_string(), t_begin_s: f.out_begin as f64 / r, t_end_s: f.out_end as f64 / r, hit_eos: f.hit_eos != 0 }).collect();
            let rate = out.sample_rate as u32;
            q3tts_long_result_free(&mut out);
            Ok((AudioSample { samples, sample_rate: rate, channels: 1 }, table))
        }
    }
}
impl TtsEngine {
    /// run_inference_stream with `stream_tx = Some(..)` — src/tts/engine.rs:444-448,520-526: every decoded 4-frame chunk is sent
    /// down the channel as soon as its PCM is on the host (`stx.send(samples.clone())`, send errors ignored as there), and the whole
    /// utterance is returned at the end. The reference threads `stream_tx` through privately (:438-443 pass None); this is the
    /// same hook made callable. Chunks come from q3tts_stream_poll; the engine overlaps the vocoder with the next frames itself.
    pub fn generate_with_voice_stream(&mut self, text_ids: &[u32], voice: &VoiceFile, instruct_ids: Option<&[u32]>,
                                      stream_tx: Option<std::sync::mpsc::Sender<Vec<f32>>>) -> Result<AudioSample, String> {
        let codes32: Vec<i32> = voice.audio_codes.iter().map(|&c| c as i32).collect();
        let desc = q3tts_prompt_desc {
            text_ids: text_ids.as_ptr(), n_text: text_ids.len() as i32,
            instruct_ids: instruct_ids.map_or(std::ptr::null(), |s| s.as_ptr()), n_instruct: instruct_ids.map_or(0, |s| s.len() as i32),
            lang_id: 2055, spk_id: -1, spk_emb: voice.speaker_embedding.as_ptr(),
            ref_codes: if codes32.is_empty() { std::ptr::null() } else { codes32.as_ptr() }, n_ref_frames: (codes32.len() / 16) as i32,
            ref_text_ids: std::ptr::null(), n_ref_text: 0,
        };
        let req = q3tts_request {
            prompt_embd: std::ptr::null(), n_tok: 0, prompt: &desc, use_engine_sampler: 0,
            temperature: self.sampler.temperature, top_k: self.sampler.top_k, top_p: self.sampler.top_p,
            has_seed: self.sampler.seed.is_some() as i32, seed: self.sampler.seed.unwrap_or(0),
            max_steps: self.max_steps as i32, min_frames: 0, force_eos_at: -1, want_pcm: 1, prefix: std::ptr::null(), text_stream: 0, text_open: 0,
        };
        unsafe {
            let err = |e: *mut q3tts_engine| CStr::from_ptr(q3tts_last_error(e)).to_string_lossy().into_owned();
            let mut st: *mut q3tts_stream = std::ptr::null_mut();
            if q3tts_stream_begin(self.raw, &req, &mut st) != 0 { return Err(err(self.raw)); }
            let mut full_audio: Vec<f32> = Vec::new();
            loop {
                let (mut chunk, mut n, mut fin) = (std::ptr::null::<c_float>(), 0i32, 0i32);
                if q3tts_stream_poll(st, &mut chunk, &mut n, &mut fin) != 0 { q3tts_stream_end(st, std::ptr::null_mut()); return Err(err(self.raw)); }
                if n > 0 {
                    let samples = std::slice::from_raw_parts(chunk, n as usize).to_vec();  // the chunk is only valid until the next poll
                    if let Some(ref stx) = stream_tx { let _ = stx.send(samples.clone()); }
                    full_audio.extend(samples);
                }
                if fin != 0 { break; }
            }
            if q3tts_stream_end(st, std::ptr::null_mut()) != 0 { return Err(err(self.raw)); }
            Ok(AudioSample { samples: full_audio, sample_rate: 24000, channels: 1 })
        }
    }
}
impl TtsEngine {
    /// The encoder half of create_voice_file (src/tts/engine.rs:375-386): 24 kHz mono samples -> VoiceFile. WAV decoding
    /// (hound, :339-373) stays in the crate.
    pub fn create_voice_from_samples(&mut self, audio: &[f32], ref_text: String) -> Result<VoiceFile, String> {
        unsafe {
            let cap = q3tts_clone_audio_frames(self.raw, audio.len() as i64).max(1);
            let mut codes = vec![0i64; cap as usize * 16];
            let mut nf = 0i32;
            let err = |e: *mut q3tts_engine| CStr::from_ptr(q3tts_last_error(e)).to_string_lossy().into_owned();
            if q3tts_clone_audio_encode(self.raw, audio.as_ptr(), audio.len() as i64, codes.as_mut_ptr(), cap, &mut nf) != 0 { return Err(err(self.raw)); }
            codes.truncate(nf as usize * 16);
            let mut emb = vec![0f32; 2048];
            if q3tts_clone_speaker_encode(self.raw, audio.as_ptr(), audio.len() as i64, emb.as_mut_ptr()) != 0 { return Err(err(self.raw)); }
            Ok(VoiceFile { ref_text, audio_codes: codes, speaker_embedding: emb })
        }
    }
}
impl Drop for TtsEngine { fn drop(&mut self) { unsafe { q3tts_engine_destroy(self.raw) } } }
/// qwen3_tts::cleanup() (src/lib.rs:18-20): nothing global to free.
pub fn cleanup() {}
