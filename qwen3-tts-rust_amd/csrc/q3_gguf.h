// q3_gguf.h — read-only GGUF (v2/v3) and NPY readers for real model files.
//
// Replaces, on the host side of libq3tts:
//   * the crate's own minimal GGUF reader for qwen3_assets.gguf (/root/reference/src/assets_manager.rs:28-265) and its NPY
//     fallback (:267-381) — same tensor / file names, same "text_embd may be absent" rule;
//   * llama.cpp's model loader for qwen3_tts_talker.gguf / qwen3_tts_predictor.gguf (behind LlamaModel::load,
//     /root/reference/src/models/llama/mod.rs:360-398), for the tensor types the released quant dirs use that this engine
//     can take: F32, F16, BF16, Q8_0 and the K-quants Q4_K / Q5_K / Q6_K of the gguf_q5_k_m directory (src/tts/engine.rs:91-95);
//     every type is de-quantised on the host and stored as bf16 (the decoder's weight format), other types are refused loudly.
// Files are mmap'ed; tensors are converted on the host and uploaded by the engine (q3_weights.hip).
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

enum { Q3_GGML_F32 = 0, Q3_GGML_F16 = 1, Q3_GGML_Q8_0 = 8, Q3_GGML_Q4_K = 12, Q3_GGML_Q5_K = 13, Q3_GGML_Q6_K = 14, Q3_GGML_BF16 = 30 };

struct Q3GgufTensor {
    std::string name;
    uint32_t type = 0;
    std::vector<uint64_t> dims;  // ne[0] is the contiguous (input / K) dimension, as in ggml
    uint64_t offset = 0;         // relative to the data section
    size_t nelem = 0, nbytes = 0;
    const uint8_t* data = nullptr;
};

// GGUF metadata value types (the file's own ids)
enum { Q3_GV_U8 = 0, Q3_GV_I8, Q3_GV_U16, Q3_GV_I16, Q3_GV_U32, Q3_GV_I32, Q3_GV_F32, Q3_GV_BOOL, Q3_GV_STR, Q3_GV_ARR, Q3_GV_U64, Q3_GV_I64, Q3_GV_F64 };
enum { Q3_META_OK = 0, Q3_META_MISSING = 1, Q3_META_TYPE = 2 };
struct Q3GgufMeta {
    uint32_t type = 0;       // Q3_GV_*
    uint32_t elem_type = 0;  // arrays: the element type (never Q3_GV_ARR: nested arrays are refused at open); else == type
    uint64_t count = 1;      // arrays: elements; else 1
    size_t off = 0, end = 0; // payload [off, end) in the mapping (see Q3Gguf::meta_raw)
};

class Q3Gguf {
public:
    Q3Gguf() = default;
    ~Q3Gguf();
    Q3Gguf(const Q3Gguf&) = delete;
    Q3Gguf& operator=(const Q3Gguf&) = delete;
    // 0 on success; err receives the reason otherwise (never throws, never aborts)
    int open(const std::string& path, std::string& err);
    const Q3GgufTensor* find(const std::string& name) const;
    const std::vector<Q3GgufTensor>& tensors() const { return tensors_; }
    uint32_t version() const { return version_; }
    uint32_t alignment() const { return alignment_; }
    // integer / bool scalar metadata widened to 64 bits (signed types sign-extended); false when absent or of another type
    bool meta_u64(const std::string& key, uint64_t* v) const;
    // Typed metadata: every KV of the file is kept as (type, count, offsets into the mapping) and decoded on access, so a
    // 150k-entry tokenizer.ggml.tokens costs one bounds-checked walk at open() and no copy. An accessor takes exactly its own class of
    // GGUF types and never coerces: Q3_META_MISSING when the key is absent, Q3_META_TYPE when it holds another type.
    bool meta_info(const std::string& key, Q3GgufMeta* out) const;
    int meta_int(const std::string& key, int64_t* v) const;        // u8 .. u64, i8 .. i64 (a u64 above INT64_MAX is Q3_META_TYPE)
    int meta_float(const std::string& key, double* v) const;       // f32, f64
    int meta_str(const std::string& key, std::string* v) const;    // string
    int meta_int_array(const std::string& key, std::vector<int64_t>* v) const;   // array of an integer type
    int meta_float_array(const std::string& key, std::vector<double>* v) const;  // array of f32 / f64
    // the payload bytes of a value inside the mapping: a scalar's bytes, a string's bytes (without its length), an array's elements as
    // the file stores them (string elements keep their u64 length prefixes); nullptr when absent
    const uint8_t* meta_raw(const std::string& key, size_t* nbytes) const;

private:
    void* map_ = nullptr;
    size_t size_ = 0;
    uint32_t version_ = 0, alignment_ = 32;
    std::vector<Q3GgufTensor> tensors_;
    std::map<std::string, size_t> index_;
    std::map<std::string, Q3GgufMeta> meta_;
};

// element conversions (ggml semantics: F16 -> f32 exact, Q8_0: f32(d) * q, BF16 -> f32 exact, K-quants: dequantize_row_q{4,5,6}_K)
int q3_gguf_to_f32(const Q3GgufTensor& t, float* dst, std::string& err);
// to bf16 with round-to-nearest-even from the f32 value above (BF16 sources are copied bit for bit)
int q3_gguf_to_bf16(const Q3GgufTensor& t, uint16_t* dst, std::string& err);

// NPY v1/v2, little-endian f32, C order (the reference assumes exactly that: src/assets_manager.rs:302-377)
int q3_npy_load_f32(const std::string& path, std::vector<float>& out, std::vector<size_t>& shape, std::string& err);
// the same header checks, shape only (the data is not read)
int q3_npy_shape(const std::string& path, std::vector<size_t>& shape, std::string& err);

// ---- the vocoder's weights file qwen3_tts_vocoder.gguf -------------------------------------------------------------------
// Tensor names and layouts are the state_dict keys and PyTorch layouts of the model family's module (transformers' Qwen3OmniMoeCode2Wav)
// plus codebook.{q}.weight and pre_conv.conv.*; every relayout to the device's arrays happens here, on the host, and the vocoder's one
// creation path (q3_voc_create) takes each array either from the seeded generator or from q3_voc_file_array.
struct q3tts_vocoder_config;
// tensor ids of the vocoder's synthetic generator (oracle/q3_oracle_vocoder.c): component, tensor of the component
enum { VC_CODEBOOK = 0, VC_PRE = 32, VC_TFM = 40, VC_FINAL_NORM = 60, VC_UP = 64, VC_DEC_IN = 72, VC_BLK = 80, VC_OUT = 120 };
enum { VW_W = 0, VW_B = 1, VW_IN_NORM = 2, VW_Q = 3, VW_K = 4, VW_V = 5, VW_O = 6, VW_LS_ATTN = 7, VW_POST_NORM = 8, VW_GATE = 9,
       VW_UP = 10, VW_DOWN = 11, VW_LS_MLP = 12, VW_DW_W = 13, VW_DW_B = 14, VW_LN_W = 15, VW_LN_B = 16, VW_PW1 = 17, VW_PW1_B = 18,
       VW_PW2 = 19, VW_PW2_B = 20, VW_GAMMA = 21, VW_ALPHA = 22, VW_BETA = 23, VW_W2 = 24, VW_B2 = 25, VW_ALPHA2 = 26, VW_BETA2 = 27 };
#define Q3_VOC_FILE_NAME "qwen3_tts_vocoder.gguf"
// wdir/qwen3_tts_vocoder.gguf (the quant directory), else the same name in wdir's parent (the model directory); "" when neither exists
std::string q3_voc_file_find(const std::string& wdir);
// The three calls below return 0, or -1 with the reason in err (it names `file` and the tensor or key).
// every field of *vc the metadata states (layer_scale_init is left alone), cross-checked against the shapes of every tensor
int q3_voc_file_config(const Q3Gguf& g, const std::string& file, q3tts_vocoder_config* vc, std::string& err);
// what q3tts_engine_create refuses before it touches the device: metadata that disagrees with vc, a missing tensor, a shape that
// disagrees with vc, an unsupported tensor type, a value that is not finite
int q3_voc_file_check(const Q3Gguf& g, const std::string& file, const q3tts_vocoder_config& vc, std::string& err);
// the array the device holds for generator id (comp, which), as f32 in device layout: matrices, convolutions and codebooks rounded to
// nearest-even bf16 (a BF16 source passes bit for bit), vectors as stored, a SnakeBeta id evaluated in double (exp(alpha),
// 1 / (exp(beta) + 1e-9)) like the generator's
int q3_voc_file_array(const Q3Gguf& g, const std::string& file, const q3tts_vocoder_config& vc, int comp, int which, std::vector<float>& out, std::string& err);

// ---- the clone encoders' weights files -------------------------------------------------------------------------------------
// Two files beside the model, found like the vocoder's: qwen3_tts_speaker_encoder.gguf (ECAPA speaker encoder) and
// qwen3_tts_codec_encoder.gguf (Mimi-style audio encoder). Tensor names and layouts are the state_dict keys and PyTorch layouts of the family's
// modules (transformers' ECAPA_TimeDelayNet and MimiModel) plus quantizer.codebook.{q}.weight; every relayout to the device's arrays happens
// here, on the host, and the encoders' one creation path (q3_clone.hip) takes each array either from the seeded generator or from
// q3_clone_file_array.
struct q3tts_clone_config;
// tensor ids of the encoders' synthetic generator (oracle/q3_oracle_clone.c): component, tensor of the component
enum { SC_TDNN0 = 0, SC_BLOCK = 1, SC_MFA = 8, SC_ASP_TDNN = 9, SC_ASP_CONV = 10, SC_FC = 11, AC_CONV0 = 32, AC_STAGE = 33,
       AC_LAST = 60, AC_TFM = 64, AC_DOWN = 100, AC_SEM_PROJ = 101, AC_AC_PROJ = 102, AC_CODEBOOK = 110 };
enum { SW_TDNN1 = 0, SW_TDNN2 = 2, SW_SE1 = 4, SW_SE2 = 6, SW_RES2 = 16 };
enum { TW_LN1_W = 0, TW_LN1_B, TW_QKV, TW_O, TW_LS1, TW_LN2_W, TW_LN2_B, TW_FC1, TW_FC2, TW_LS2 };
#define Q3_SPK_FILE_NAME "qwen3_tts_speaker_encoder.gguf"
#define Q3_CODEC_FILE_NAME "qwen3_tts_codec_encoder.gguf"
struct Q3CloneFiles { Q3Gguf spk, codec; std::string spk_path, codec_path; };
// Finds each file in wdir (the quant directory), else in wdir's parent, and opens both. 0; 1 when a file is not found (err names it, and
// says which of the two was there); 2 when a file that was found cannot be opened or ends early.
int q3_clone_files_open(const std::string& wdir, Q3CloneFiles& f, std::string& err);
// The three calls below return 0, or -1 with the reason in err (it names the file and the tensor or key).
// every field of *cc the metadata states (ae_layer_scale is left alone), cross-checked against the shapes of every tensor; *cc is
// written only on success
int q3_clone_file_config(const Q3CloneFiles& f, q3tts_clone_config* cc, std::string& err);
// what q3tts_clone_load refuses beyond that before it touches the device: a value that is not finite
int q3_clone_file_check(const Q3CloneFiles& f, const q3tts_clone_config& cc, std::string& err);
// the array the device holds for generator id (comp, which), as f32 in device layout: a convolution or projection [n][cin][k] as the rows
// W[n][tap * cin + ci], zero-padded to round512(k * cin) and rounded to nearest-even bf16 (a BF16 source passes bit for bit), q / k / v
// fused into the QKV rows in that order; biases, LayerNorm, LayerScale and codebooks as stored
int q3_clone_file_array(const Q3CloneFiles& f, const q3tts_clone_config& cc, int comp, int which, std::vector<float>& out, std::string& err);
