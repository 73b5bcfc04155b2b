// q3_model_dir.cpp — q3tts_config_from_model_dir: every model dimension of an engine configuration from the files of a quant
// directory (host only, no GPU). What llama.cpp reads from the two GGUFs and hands to the reference crate
// (reference: src/models/llama/mod.rs:348-353, src/tts/engine.rs:84-137), plus the table shapes of the assets
// (src/assets_manager.rs:212-249). The contract is in include/q3tts.h; the key table in DESIGN.md §11.
#include <dirent.h>
#include <sys/stat.h>

#include <cstdio>
#include <cstring>
#include <set>

#include "../../include/q3tts.h"
#include "q3_gguf.h"

namespace {

struct Fail {
    int code = Q3TTS_OK; std::string msg;
    int set(int c, const std::string& m) { code = c; msg = m; return c; }
};

bool file_exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); }

// what one transformer's file states
struct Tfm { int64_t L = 0, d = 0, F = 0, H = 0, Hkv = 0, hd = 0, head_rows = 0; float theta = 10000.0f, eps = 0.0f; };

struct Reader {
    const Q3Gguf& g; const std::string file; std::string arch; Fail& f;
    std::string key(const char* suffix) const { return arch + "." + suffix; }
    int missing(const std::string& k) { return f.set(Q3TTS_ERR_INVALID, file + ": metadata key '" + k + "' is missing"); }
    int wrong_type(const std::string& k, const char* want) {
        Q3GgufMeta m; g.meta_info(k, &m);
        return f.set(Q3TTS_ERR_INVALID, file + ": metadata key '" + k + "' is not " + want + " (GGUF value type " + std::to_string(m.type) +
                                            (m.type == Q3_GV_ARR ? " of " + std::to_string(m.elem_type) : std::string()) + ")");
    }
    // a count: an integer in 1 .. 2^31 - 1
    int count(const std::string& k, bool required, int64_t* v, bool* present = nullptr) {
        const int st = g.meta_int(k, v);
        if (present) *present = st == Q3_META_OK;
        if (st == Q3_META_MISSING) return required ? missing(k) : Q3TTS_OK;
        if (st == Q3_META_TYPE) return wrong_type(k, "an integer");
        if (*v < 1 || *v > INT32_MAX) return f.set(Q3TTS_ERR_INVALID, file + ": metadata key '" + k + "' = " + std::to_string(*v) + " is out of range");
        return Q3TTS_OK;
    }
    int real(const std::string& k, bool required, float* v) {
        double d = 0;
        const int st = g.meta_float(k, &d);
        if (st == Q3_META_MISSING) return required ? missing(k) : Q3TTS_OK;
        if (st == Q3_META_TYPE) return wrong_type(k, "a float");
        *v = (float)d;
        return Q3TTS_OK;
    }
    // tensor `name` must be [rows][cols]; rows_key / cols_key are the metadata keys those numbers came from
    int shape(const std::string& name, int64_t rows, const std::string& rows_key, int64_t cols, const std::string& cols_key) {
        const Q3GgufTensor* t = g.find(name);
        if (!t) return f.set(Q3TTS_ERR_INVALID, file + ": tensor '" + name + "' is missing");
        const int64_t c = (int64_t)t->dims[0], r = t->dims.size() > 1 ? (int64_t)t->dims[1] : 1;
        if (t->dims.size() > 2) return f.set(Q3TTS_ERR_INVALID, file + ": tensor '" + name + "' is not a matrix");
        if (r != rows) return f.set(Q3TTS_ERR_INVALID, file + ": tensor '" + name + "' has " + std::to_string(r) + " rows, metadata key '" + rows_key + "' implies " + std::to_string(rows));
        if (c != cols) return f.set(Q3TTS_ERR_INVALID, file + ": tensor '" + name + "' has row length " + std::to_string(c) + ", metadata key '" + cols_key + "' implies " + std::to_string(cols));
        return Q3TTS_OK;
    }
};

#define TRYF(x) do { const int rc__ = (x); if (rc__ != Q3TTS_OK) return rc__; } while (0)

int read_tfm(const Q3Gguf& g, const std::string& file, bool talker, Tfm* t, int32_t* sections, Fail& f) {
    Reader r{g, file, std::string(), f};
    const int st = g.meta_str("general.architecture", &r.arch);
    if (st == Q3_META_MISSING) return r.missing("general.architecture");
    if (st == Q3_META_TYPE) return r.wrong_type("general.architecture", "a string");
    const std::string kL = r.key("block_count"), kd = r.key("embedding_length"), kF = r.key("feed_forward_length"), kH = r.key("attention.head_count"),
                      kHkv = r.key("attention.head_count_kv"), khd = r.key("attention.key_length"), kth = r.key("rope.freq_base"),
                      keps = r.key("attention.layer_norm_rms_epsilon"), ksec = r.key("rope.dimension_sections");
    TRYF(r.count(kL, true, &t->L));
    TRYF(r.count(kd, true, &t->d));
    TRYF(r.count(kF, true, &t->F));
    TRYF(r.count(kH, true, &t->H));
    TRYF(r.count(kHkv, true, &t->Hkv));
    bool have_hd = false;
    TRYF(r.count(khd, false, &t->hd, &have_hd));
    if (!have_hd) t->hd = t->d / t->H;  // llama.cpp's rule: n_embd / n_head
    if (t->hd < 1 || t->H * t->hd > INT32_MAX || t->Hkv * t->hd > INT32_MAX) return f.set(Q3TTS_ERR_INVALID, file + ": metadata key '" + khd + "' is out of range");
    t->theta = 10000.0f;
    TRYF(r.real(kth, false, &t->theta));
    TRYF(r.real(keps, true, &t->eps));
    if (talker) {
        std::vector<int64_t> sec;
        const int ss = g.meta_int_array(ksec, &sec);
        if (ss == Q3_META_MISSING) return r.missing(ksec);
        if (ss == Q3_META_TYPE) return r.wrong_type(ksec, "an integer array");
        if (sec.empty() || sec.size() > 4) return f.set(Q3TTS_ERR_INVALID, file + ": metadata key '" + ksec + "' has " + std::to_string(sec.size()) + " entries, 1 .. 4 are allowed");
        int64_t sum = 0;
        for (size_t i = 0; i < 4; ++i) {
            const int64_t v = i < sec.size() ? sec[i] : 0;
            if (v < 0 || v > t->hd) return f.set(Q3TTS_ERR_INVALID, file + ": metadata key '" + ksec + "' entry " + std::to_string(i) + " = " + std::to_string(v) + " is out of range");
            sections[i] = (int32_t)v; sum += v;
        }
        if (sum != t->hd / 2) return f.set(Q3TTS_ERR_INVALID, file + ": metadata key '" + ksec + "' sums to " + std::to_string(sum) + ", head_dim / 2 is " + std::to_string(t->hd / 2));
    }
    // the first block's matrices and the head against what the metadata implies
    TRYF(r.shape("blk.0.attn_q.weight", t->H * t->hd, kH, t->d, kd));
    TRYF(r.shape("blk.0.attn_k.weight", t->Hkv * t->hd, kHkv, t->d, kd));
    TRYF(r.shape("blk.0.attn_output.weight", t->d, kd, t->H * t->hd, kH));
    TRYF(r.shape("blk.0.ffn_gate.weight", t->F, kF, t->d, kd));
    TRYF(r.shape("blk.0.ffn_down.weight", t->d, kd, t->F, kF));
    const Q3GgufTensor* head = g.find("output.weight");
    if (!head) return f.set(Q3TTS_ERR_INVALID, file + ": tensor 'output.weight' is missing");
    if (head->dims.size() != 2) return f.set(Q3TTS_ERR_INVALID, file + ": tensor 'output.weight' is not a matrix");
    if ((int64_t)head->dims[0] != t->d)
        return f.set(Q3TTS_ERR_INVALID, file + ": tensor 'output.weight' has row length " + std::to_string(head->dims[0]) + ", metadata key '" + kd + "' implies " + std::to_string(t->d));
    if (head->dims[1] > (uint64_t)INT32_MAX) return f.set(Q3TTS_ERR_INVALID, file + ": tensor 'output.weight' has too many rows");
    t->head_rows = (int64_t)head->dims[1];
    return Q3TTS_OK;
}

// shapes of the asset tables: [rows][cols] per name; rows = -1 when absent
struct Table { int64_t rows = -1, cols = 0; };

// indices N of the entries "<prefix>N<suffix>" must be 0 .. n - 1
int contiguous(const std::set<int64_t>& idx, const std::string& where, const std::string& prefix, const std::string& suffix, Fail& f) {
    int64_t want = 0;
    for (int64_t i : idx) {
        if (i != want) return f.set(Q3TTS_ERR_INVALID, where + ": '" + prefix + std::to_string(want) + suffix + "' is missing ('" + prefix + std::to_string(i) + suffix + "' exists: the codec tables must be contiguous from 0)");
        ++want;
    }
    return Q3TTS_OK;
}

bool parse_index(const std::string& s, size_t from, size_t to, int64_t* v) {
    if (from >= to || to - from > 9) return false;
    int64_t x = 0;
    for (size_t i = from; i < to; ++i) { if (s[i] < '0' || s[i] > '9') return false; x = x * 10 + (s[i] - '0'); }
    if (to - from > 1 && s[from] == '0') return false;  // "01" is not table 1
    *v = x;
    return true;
}

int read_assets(const std::string& dir, std::string* where, Table* proj, Table* text, std::vector<Table>* codec, std::string* codec_prefix, std::string* codec_suffix, Fail& f) {
    const std::string gpath = dir + "/qwen3_assets.gguf";
    std::string err;
    if (file_exists(gpath)) {
        *where = "qwen3_assets.gguf"; *codec_prefix = "codec_embd."; *codec_suffix = "";
        Q3Gguf g;
        if (g.open(gpath, err)) return f.set(Q3TTS_ERR_IO, err);
        std::set<int64_t> idx;
        for (const Q3GgufTensor& t : g.tensors()) {
            int64_t i;
            if (t.name.compare(0, 11, "codec_embd.") == 0 && parse_index(t.name, 11, t.name.size(), &i)) idx.insert(i);
        }
        TRYF(contiguous(idx, *where, *codec_prefix, *codec_suffix, f));
        auto get = [&](const std::string& name, Table* out) -> int {
            const Q3GgufTensor* t = g.find(name);
            if (!t) return Q3TTS_OK;
            if (t->dims.size() != 2 || t->dims[0] > (uint64_t)INT32_MAX || t->dims[1] > (uint64_t)INT32_MAX) return f.set(Q3TTS_ERR_INVALID, *where + ": tensor '" + name + "' is not a matrix");
            out->cols = (int64_t)t->dims[0]; out->rows = (int64_t)t->dims[1];
            return Q3TTS_OK;
        };
        TRYF(get("proj.weight", proj));
        TRYF(get("text_embd", text));
        codec->resize(idx.size());
        for (size_t q = 0; q < idx.size(); ++q) TRYF(get("codec_embd." + std::to_string(q), &(*codec)[q]));
        return Q3TTS_OK;
    }
    // the legacy NPY layout (src/assets_manager.rs:267-300)
    *where = "NPY assets"; *codec_prefix = "codec_embedding_"; *codec_suffix = ".npy";
    std::set<int64_t> idx;
    if (DIR* dp = opendir(dir.c_str())) {
        while (const dirent* de = readdir(dp)) {
            const std::string n = de->d_name;
            int64_t i;
            if (n.size() > 20 && n.compare(0, 16, "codec_embedding_") == 0 && n.compare(n.size() - 4, 4, ".npy") == 0 && parse_index(n, 16, n.size() - 4, &i)) idx.insert(i);
        }
        closedir(dp);
    }
    if (idx.empty()) return f.set(Q3TTS_ERR_IO, "neither qwen3_assets.gguf nor codec_embedding_0.npy in " + dir);
    TRYF(contiguous(idx, *where, *codec_prefix, *codec_suffix, f));
    auto get = [&](const std::string& file, Table* out) -> int {
        const std::string path = dir + "/" + file;
        if (!file_exists(path)) return Q3TTS_OK;
        std::vector<size_t> shape;
        if (q3_npy_shape(path, shape, err)) return f.set(Q3TTS_ERR_IO, err);
        if (shape.size() != 2 || shape[0] > (size_t)INT32_MAX || shape[1] > (size_t)INT32_MAX) return f.set(Q3TTS_ERR_INVALID, *where + ": '" + file + "' is not a matrix");
        out->rows = (int64_t)shape[0]; out->cols = (int64_t)shape[1];
        return Q3TTS_OK;
    };
    TRYF(get("proj_weight.npy", proj));
    TRYF(get("text_embedding_projected.npy", text));
    codec->resize(idx.size());
    for (size_t q = 0; q < idx.size(); ++q) TRYF(get("codec_embedding_" + std::to_string(q) + ".npy", &(*codec)[q]));
    return Q3TTS_OK;
}

int from_dir(const std::string& dir, q3tts_model_config* m, Fail& f) {
    static const char* kTalker = "qwen3_tts_talker.gguf";
    static const char* kPred = "qwen3_tts_predictor.gguf";
    for (const char* name : {kTalker, kPred})
        if (!file_exists(dir + "/" + name)) return f.set(Q3TTS_ERR_IO, "cannot open " + dir + "/" + name + ": no such file");
    std::string err;
    Tfm T, P;
    int32_t sections[4] = {0, 0, 0, 0};
    std::string t_dkey;
    {
        Q3Gguf g;
        if (g.open(dir + "/" + kTalker, err)) return f.set(Q3TTS_ERR_IO, err);
        TRYF(read_tfm(g, kTalker, true, &T, sections, f));
        std::string arch; g.meta_str("general.architecture", &arch);
        t_dkey = arch + ".embedding_length";
    }
    std::string p_dkey;
    {
        Q3Gguf g;
        if (g.open(dir + "/" + kPred, err)) return f.set(Q3TTS_ERR_IO, err);
        TRYF(read_tfm(g, kPred, false, &P, nullptr, f));
        std::string arch; g.meta_str("general.architecture", &arch);
        p_dkey = arch + ".embedding_length";
        if (P.eps != T.eps) {
            char a[32], b[32]; snprintf(a, sizeof a, "%g", (double)T.eps); snprintf(b, sizeof b, "%g", (double)P.eps);
            return f.set(Q3TTS_ERR_INVALID, std::string(kPred) + ": metadata key '" + arch + ".attention.layer_norm_rms_epsilon' = " + b + " differs from " + kTalker + "'s " + a + " (rms_eps is one value for both)");
        }
    }
    std::string where, cpre, csuf;
    Table proj, text; std::vector<Table> codec;
    TRYF(read_assets(dir, &where, &proj, &text, &codec, &cpre, &csuf, f));
    auto cname = [&](size_t q) { return "'" + cpre + std::to_string(q) + csuf + "'"; };
    const int64_t ncb = (int64_t)codec.size();
    if (ncb < 2) return f.set(Q3TTS_ERR_INVALID, where + ": " + std::to_string(ncb) + " codec table(s) (" + cname(0) + " ...), at least 2 are needed");
    const int64_t d_embed = codec[0].cols;
    if (d_embed != T.d)
        return f.set(Q3TTS_ERR_INVALID, where + ": " + cname(0) + " has row length " + std::to_string(d_embed) + ", " + kTalker + "'s metadata key '" + t_dkey + "' implies " + std::to_string(T.d));
    for (size_t q = 1; q < codec.size(); ++q) {
        if (codec[q].cols != d_embed) return f.set(Q3TTS_ERR_INVALID, where + ": " + cname(q) + " has row length " + std::to_string(codec[q].cols) + ", " + cname(0) + " has " + std::to_string(d_embed));
        if (codec[q].rows != codec[1].rows) return f.set(Q3TTS_ERR_INVALID, where + ": " + cname(q) + " has " + std::to_string(codec[q].rows) + " rows, " + cname(1) + " has " + std::to_string(codec[1].rows));
    }
    if (text.rows >= 0 && text.cols != d_embed) return f.set(Q3TTS_ERR_INVALID, where + ": the text table has row length " + std::to_string(text.cols) + ", " + cname(0) + " has " + std::to_string(d_embed));
    const std::string pname = csuf.empty() ? "proj.weight" : "proj_weight.npy";
    if (proj.rows < 0) return f.set(Q3TTS_ERR_INVALID, where + ": '" + pname + "' is missing");
    if (proj.rows != P.d) return f.set(Q3TTS_ERR_INVALID, where + ": '" + pname + "' has " + std::to_string(proj.rows) + " rows, " + kPred + "'s metadata key '" + p_dkey + "' implies " + std::to_string(P.d));
    if (proj.cols != d_embed) return f.set(Q3TTS_ERR_INVALID, where + ": '" + pname + "' has row length " + std::to_string(proj.cols) + ", " + cname(0) + " has " + std::to_string(d_embed));
    if (P.head_rows % (ncb - 1))
        return f.set(Q3TTS_ERR_INVALID, std::string(kPred) + ": tensor 'output.weight' has " + std::to_string(P.head_rows) + " rows, not a multiple of n_codebooks - 1 = " + std::to_string(ncb - 1) + " (" + where + " holds " + std::to_string(ncb) + " codec tables)");
    m->t_n_layer = (int32_t)T.L; m->t_d_model = (int32_t)T.d; m->t_n_head = (int32_t)T.H; m->t_n_kv_head = (int32_t)T.Hkv; m->t_head_dim = (int32_t)T.hd;
    m->t_d_ffn = (int32_t)T.F; m->t_vocab = (int32_t)T.head_rows; m->t_rope_theta = T.theta;
    for (int i = 0; i < 4; ++i) m->t_mrope_sections[i] = sections[i];
    m->p_n_layer = (int32_t)P.L; m->p_d_model = (int32_t)P.d; m->p_n_head = (int32_t)P.H; m->p_n_kv_head = (int32_t)P.Hkv; m->p_head_dim = (int32_t)P.hd;
    m->p_d_ffn = (int32_t)P.F; m->p_rope_theta = P.theta;
    m->n_codebooks = (int32_t)ncb; m->codebook_size = (int32_t)(P.head_rows / (ncb - 1));
    m->rms_eps = T.eps;
    m->d_embed = (int32_t)d_embed; m->text_vocab = text.rows < 0 ? 0 : (int32_t)text.rows;
    m->codec0_rows = (int32_t)codec[0].rows; m->codecq_rows = (int32_t)codec[1].rows;
    return Q3TTS_OK;
}

}  // namespace

extern "C" int q3tts_config_from_model_dir(const char* model_dir, const char* quant, q3tts_engine_config* cfg, char* path_buf, int32_t path_cap,
                                           char* err, int32_t err_cap) {
    Fail f;
    auto done = [&](int rc) {
        if (err && err_cap > 0) { const size_t n = f.msg.size() < (size_t)err_cap - 1 ? f.msg.size() : (size_t)err_cap - 1; memcpy(err, f.msg.data(), n); err[n] = '\0'; }
        return rc;
    };
    if (!model_dir || !cfg || !path_buf) return done(f.set(Q3TTS_ERR_INVALID, "null argument"));
    const char* qd = "gguf";  // src/tts/engine.rs:91-95
    if (quant && !strcmp(quant, "q5_k_m")) qd = "gguf_q5_k_m";
    else if (quant && !strcmp(quant, "q8_0")) qd = "gguf_q8_0";
    const std::string dir = std::string(model_dir) + "/" + qd;
    if (path_cap < 0 || (size_t)path_cap < dir.size() + 1) return done(f.set(Q3TTS_ERR_INVALID, "path_buf holds " + std::to_string(path_cap) + " bytes, " + std::to_string(dir.size() + 1) + " are needed"));
    q3tts_model_config m = cfg->model;  // cfg itself is written only on success
    const int rc = from_dir(dir, &m, f);
    if (rc != Q3TTS_OK) return done(rc);
    // the vocoder's shape from its own file, found by the engine's rule (q3_voc_file_find); without one the block is left alone
    q3tts_vocoder_config vc = cfg->vocoder;
    const std::string vfile = cfg->with_vocoder ? q3_voc_file_find(dir) : std::string();
    if (!vfile.empty()) {
        Q3Gguf g;
        std::string er;
        if (g.open(vfile, er)) return done(f.set(Q3TTS_ERR_IO, er));
        if (q3_voc_file_config(g, vfile, &vc, er)) return done(f.set(Q3TTS_ERR_INVALID, er));
    }
    memcpy(path_buf, dir.c_str(), dir.size() + 1);
    cfg->model = m;
    cfg->vocoder = vc;
    cfg->weights_path = path_buf;
    return done(Q3TTS_OK);
}
