// q3_gguf.cpp — GGUF v2/v3 + NPY readers (host only). See q3_gguf.h for what they replace in the reference.
#include "q3_gguf.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstring>

namespace {

struct Cursor {
    const uint8_t* p; size_t n, pos;
    bool take(void* dst, size_t k) {
        if (k > n - pos) return false;
        memcpy(dst, p + pos, k); pos += k;
        return true;
    }
    bool skip(size_t k) { if (k > n - pos) return false; pos += k; return true; }
    template <class T> bool get(T* v) { return take(v, sizeof(T)); }
    bool str(std::string* s) {
        uint64_t len = 0;
        if (!get(&len) || len > n - pos) return false;
        s->assign((const char*)p + pos, (size_t)len); pos += (size_t)len;
        return true;
    }
    bool skip_str() {  // a string that is only walked over (metadata values stay in the mapping)
        uint64_t len = 0;
        return get(&len) && skip_checked(len);
    }
    bool skip_checked(uint64_t k) { if (k > n - pos) return false; pos += (size_t)k; return true; }
};

size_t scalar_size(uint32_t t) {
    switch (t) {
        case Q3_GV_U8: case Q3_GV_I8: case Q3_GV_BOOL: return 1;
        case Q3_GV_U16: case Q3_GV_I16: return 2;
        case Q3_GV_U32: case Q3_GV_I32: case Q3_GV_F32: return 4;
        case Q3_GV_U64: case Q3_GV_I64: case Q3_GV_F64: return 8;
        default: return 0;
    }
}
bool is_int_type(uint32_t t) { return t == Q3_GV_U8 || t == Q3_GV_I8 || t == Q3_GV_U16 || t == Q3_GV_I16 || t == Q3_GV_U32 || t == Q3_GV_I32 || t == Q3_GV_U64 || t == Q3_GV_I64; }
bool is_float_type(uint32_t t) { return t == Q3_GV_F32 || t == Q3_GV_F64; }
// one integer (or bool) scalar at p, widened to 64 bits with its sign
uint64_t load_int(const uint8_t* p, uint32_t t) {
    switch (t) {
        case Q3_GV_I8: return (uint64_t)(int64_t)(int8_t)p[0];
        case Q3_GV_I16: { int16_t s; memcpy(&s, p, 2); return (uint64_t)(int64_t)s; }
        case Q3_GV_I32: { int32_t s; memcpy(&s, p, 4); return (uint64_t)(int64_t)s; }
        default: { uint64_t v = 0; memcpy(&v, p, scalar_size(t)); return v; }  // unsigned types, bool, i64 (little-endian host)
    }
}
double load_float(const uint8_t* p, uint32_t t) {
    if (t == Q3_GV_F32) { float f; memcpy(&f, p, 4); return (double)f; }
    double d; memcpy(&d, p, 8); return d;
}

inline float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1f, man = h & 0x3ffu;
    uint32_t u;
    if (exp == 0) {
        if (man == 0) u = sign;
        else {  // subnormal: normalise
            int e = -1; uint32_t m = man;
            do { ++e; m <<= 1; } while (!(m & 0x400u));
            u = sign | ((uint32_t)(127 - 15 - e) << 23) | ((m & 0x3ffu) << 13);
        }
    } else if (exp == 31) u = sign | 0x7f800000u | (man << 13);
    else u = sign | ((exp + 127 - 15) << 23) | (man << 13);
    float f; memcpy(&f, &u, 4);
    return f;
}
inline uint16_t f32_to_bf16_rne(float f) {  // same rounding as q3_bf16 (q3_common.h): RNE, NaN stays NaN
    uint32_t u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
size_t type_bytes(uint32_t type, size_t nelem, uint64_t ne0, bool* ok) {
    *ok = true;
    switch (type) {
        case Q3_GGML_F32: return nelem * 4;
        case Q3_GGML_F16: case Q3_GGML_BF16: return nelem * 2;
        case Q3_GGML_Q8_0: if (ne0 % 32) { *ok = false; return 0; } return nelem / 32 * 34;
        case Q3_GGML_Q4_K: if (ne0 % 256) { *ok = false; return 0; } return nelem / 256 * 144;
        case Q3_GGML_Q5_K: if (ne0 % 256) { *ok = false; return 0; } return nelem / 256 * 176;
        case Q3_GGML_Q6_K: if (ne0 % 256) { *ok = false; return 0; } return nelem / 256 * 210;
        default: *ok = false; return 0;
    }
}

// ---- ggml's K-quants (super-blocks of 256; the gguf_q5_k_m directory of the reference, src/tts/engine.rs:91-95, holds Q5_K and Q6_K
// tensors). The layouts are llama.cpp's (ggml-quants.c dequantize_row_q4_K / q5_K / q6_K), restated from their published definition:
// llama.cpp is not in /root/reference, so this row is PARITY UNPINNED; tests/_gguf.py holds the independent numpy restatement. ----
// 6-bit (scale, min) pair j of a Q4_K / Q5_K super-block (get_scale_min_k4)
inline void scale_min_k4(int j, const uint8_t* q, uint8_t* sc, uint8_t* m) {
    if (j < 4) { *sc = q[j] & 63; *m = q[j + 4] & 63; }
    else { *sc = (uint8_t)((q[j + 4] & 0xF) | ((q[j - 4] >> 6) << 4)); *m = (uint8_t)((q[j + 4] >> 4) | ((q[j] >> 6) << 4)); }
}
// one super-block -> 256 floats
void deq_q4_k(const uint8_t* b, float* y) {   // { f16 d, dmin; u8 scales[12]; u8 qs[128] }
    uint16_t h; memcpy(&h, b, 2); const float d = f16_to_f32(h); memcpy(&h, b + 2, 2); const float dmin = f16_to_f32(h);
    const uint8_t* scales = b + 4; const uint8_t* q = b + 16;
    int is = 0;
    for (int j = 0; j < 256; j += 64) {
        uint8_t sc, m;
        scale_min_k4(is + 0, scales, &sc, &m); const float d1 = d * (float)sc, m1 = dmin * (float)m;
        scale_min_k4(is + 1, scales, &sc, &m); const float d2 = d * (float)sc, m2 = dmin * (float)m;
        for (int l = 0; l < 32; ++l) *y++ = d1 * (float)(q[l] & 0xF) - m1;
        for (int l = 0; l < 32; ++l) *y++ = d2 * (float)(q[l] >> 4) - m2;
        q += 32; is += 2;
    }
}
void deq_q5_k(const uint8_t* b, float* y) {   // { f16 d, dmin; u8 scales[12]; u8 qh[32]; u8 qs[128] }
    uint16_t h; memcpy(&h, b, 2); const float d = f16_to_f32(h); memcpy(&h, b + 2, 2); const float dmin = f16_to_f32(h);
    const uint8_t* scales = b + 4; const uint8_t* qh = b + 16; const uint8_t* ql = b + 48;
    int is = 0; uint8_t u1 = 1, u2 = 2;
    for (int j = 0; j < 256; j += 64) {
        uint8_t sc, m;
        scale_min_k4(is + 0, scales, &sc, &m); const float d1 = d * (float)sc, m1 = dmin * (float)m;
        scale_min_k4(is + 1, scales, &sc, &m); const float d2 = d * (float)sc, m2 = dmin * (float)m;
        for (int l = 0; l < 32; ++l) *y++ = d1 * (float)((ql[l] & 0xF) + ((qh[l] & u1) ? 16 : 0)) - m1;
        for (int l = 0; l < 32; ++l) *y++ = d2 * (float)((ql[l] >> 4) + ((qh[l] & u2) ? 16 : 0)) - m2;
        ql += 32; is += 2; u1 = (uint8_t)(u1 << 2); u2 = (uint8_t)(u2 << 2);
    }
}
void deq_q6_k(const uint8_t* b, float* y) {   // { u8 ql[128]; u8 qh[64]; i8 scales[16]; f16 d }
    const uint8_t* ql = b; const uint8_t* qh = b + 128; const int8_t* sc = (const int8_t*)(b + 192);
    uint16_t h; memcpy(&h, b + 208, 2); const float d = f16_to_f32(h);
    for (int n = 0; n < 256; n += 128) {
        for (int l = 0; l < 32; ++l) {
            const int is = l / 16;
            const int q1 = (int)(int8_t)((ql[l + 0] & 0xF) | (((qh[l] >> 0) & 3) << 4)) - 32;
            const int q2 = (int)(int8_t)((ql[l + 32] & 0xF) | (((qh[l] >> 2) & 3) << 4)) - 32;
            const int q3 = (int)(int8_t)((ql[l + 0] >> 4) | (((qh[l] >> 4) & 3) << 4)) - 32;
            const int q4 = (int)(int8_t)((ql[l + 32] >> 4) | (((qh[l] >> 6) & 3) << 4)) - 32;
            y[l + 0] = d * (float)sc[is + 0] * (float)q1;
            y[l + 32] = d * (float)sc[is + 2] * (float)q2;
            y[l + 64] = d * (float)sc[is + 4] * (float)q3;
            y[l + 96] = d * (float)sc[is + 6] * (float)q4;
        }
        y += 128; ql += 64; qh += 32; sc += 8;
    }
}
// K-quant super-block kb of tensor t -> 256 floats; false for other types
bool deq_k_block(const Q3GgufTensor& t, size_t kb, float* y) {
    switch (t.type) {
        case Q3_GGML_Q4_K: deq_q4_k(t.data + kb * 144, y); return true;
        case Q3_GGML_Q5_K: deq_q5_k(t.data + kb * 176, y); return true;
        case Q3_GGML_Q6_K: deq_q6_k(t.data + kb * 210, y); return true;
        default: return false;
    }
}

}  // namespace

Q3Gguf::~Q3Gguf() { if (map_) munmap(map_, size_); }

int Q3Gguf::open(const std::string& path, std::string& err) {
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) { err = "cannot open " + path; return -1; }
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size < 24) { ::close(fd); err = path + ": too small for a GGUF header"; return -1; }
    size_ = (size_t)st.st_size;
    map_ = mmap(nullptr, size_, PROT_READ, MAP_PRIVATE, fd, 0);
    ::close(fd);
    if (map_ == MAP_FAILED) { map_ = nullptr; err = "mmap failed for " + path; return -1; }
    Cursor c{(const uint8_t*)map_, size_, 0};
    char magic[4];
    uint64_t n_tensors = 0, n_kv = 0;
    if (!c.take(magic, 4) || memcmp(magic, "GGUF", 4) != 0) { err = path + ": not a GGUF file"; return -1; }
    if (!c.get(&version_) || version_ < 2 || version_ > 3) {  // v1 has 32-bit counts; the reference refuses it too (:42-45)
        err = path + ": unsupported GGUF version " + std::to_string(version_); return -1;
    }
    if (!c.get(&n_tensors) || !c.get(&n_kv) || n_tensors > (1u << 24) || n_kv > (1u << 24)) { err = path + ": corrupt GGUF header"; return -1; }
    for (uint64_t i = 0; i < n_kv; ++i) {
        // a length that runs past the file names the key, or the byte offset when the key itself is cut
        const size_t key_at = c.pos;
        std::string key; Q3GgufMeta kv;
        if (!c.str(&key) || !c.get(&kv.type)) { err = path + ": metadata key at byte offset " + std::to_string(key_at) + " runs past the file"; return -1; }
        const std::string what = path + ": metadata '" + key + "'";
        kv.elem_type = kv.type; kv.off = c.pos;
        if (kv.type == Q3_GV_STR) {
            if (!c.skip_str()) { err = what + ": string length runs past the file"; return -1; }
            kv.off += 8;
        } else if (kv.type == Q3_GV_ARR) {  // (the reference's reader gives up on arrays, :93-97; real llama.cpp files have them)
            if (!c.get(&kv.elem_type) || !c.get(&kv.count)) { err = what + ": array header runs past the file"; return -1; }
            kv.off = c.pos;
            if (kv.elem_type == Q3_GV_ARR) { err = what + ": nested arrays are not supported"; return -1; }
            if (kv.elem_type == Q3_GV_STR) {
                if (kv.count > (c.n - c.pos) / 8) { err = what + ": array length " + std::to_string(kv.count) + " runs past the file"; return -1; }
                for (uint64_t j = 0; j < kv.count; ++j)
                    if (!c.skip_str()) { err = what + ": string length of element " + std::to_string(j) + " runs past the file"; return -1; }
            } else {
                const size_t es = scalar_size(kv.elem_type);
                if (!es) { err = what + ": unknown array element type " + std::to_string(kv.elem_type); return -1; }
                if (kv.count > (c.n - c.pos) / es) { err = what + ": array length " + std::to_string(kv.count) + " runs past the file"; return -1; }
                c.pos += (size_t)kv.count * es;
            }
        } else {
            const size_t es = scalar_size(kv.type);
            if (!es) { err = path + ": unknown metadata value type " + std::to_string(kv.type) + " for '" + key + "'"; return -1; }
            if (!c.skip(es)) { err = what + ": value runs past the file"; return -1; }
        }
        kv.end = c.pos;
        meta_[key] = kv;
    }
    uint64_t al = 0;
    if (meta_u64("general.alignment", &al) && al >= 1 && al <= (1u << 20) && (al & (al - 1)) == 0) alignment_ = (uint32_t)al;
    tensors_.resize((size_t)n_tensors);
    for (auto& t : tensors_) {
        uint32_t nd = 0;
        if (!c.str(&t.name) || !c.get(&nd) || nd < 1 || nd > 4) { err = path + ": bad tensor info"; return -1; }
        t.dims.resize(nd); t.nelem = 1;
        for (uint32_t d = 0; d < nd; ++d) {
            if (!c.get(&t.dims[d]) || t.dims[d] == 0 || t.dims[d] > ((uint64_t)1 << 40)) { err = path + ": bad tensor shape for '" + t.name + "'"; return -1; }
            t.nelem *= (size_t)t.dims[d];
        }
        if (!c.get(&t.type) || !c.get(&t.offset)) { err = path + ": truncated tensor info"; return -1; }
    }
    const size_t data_start = (c.pos + alignment_ - 1) / alignment_ * alignment_;
    for (size_t i = 0; i < tensors_.size(); ++i) {
        Q3GgufTensor& t = tensors_[i];
        bool ok = false;
        t.nbytes = type_bytes(t.type, t.nelem, t.dims[0], &ok);
        if (ok) {  // unsupported types stay listed (data == nullptr) and fail only if somebody asks for them
            if (t.offset % alignment_ || data_start > size_ || t.offset > size_ - data_start || t.nbytes > size_ - data_start - t.offset) {
                err = path + ": tensor '" + t.name + "' lies outside the file"; return -1;
            }
            t.data = (const uint8_t*)map_ + data_start + t.offset;
        }
        index_[t.name] = i;
    }
    return 0;
}

const Q3GgufTensor* Q3Gguf::find(const std::string& name) const {
    auto it = index_.find(name);
    return it == index_.end() ? nullptr : &tensors_[it->second];
}
bool Q3Gguf::meta_u64(const std::string& key, uint64_t* v) const {
    auto it = meta_.find(key);
    if (it == meta_.end() || !(is_int_type(it->second.type) || it->second.type == Q3_GV_BOOL)) return false;
    *v = load_int((const uint8_t*)map_ + it->second.off, it->second.type);
    return true;
}
bool Q3Gguf::meta_info(const std::string& key, Q3GgufMeta* out) const {
    auto it = meta_.find(key);
    if (it == meta_.end()) return false;
    if (out) *out = it->second;
    return true;
}
const uint8_t* Q3Gguf::meta_raw(const std::string& key, size_t* nbytes) const {
    auto it = meta_.find(key);
    if (it == meta_.end()) return nullptr;
    if (nbytes) *nbytes = it->second.end - it->second.off;
    return (const uint8_t*)map_ + it->second.off;
}
int Q3Gguf::meta_int(const std::string& key, int64_t* v) const {
    auto it = meta_.find(key);
    if (it == meta_.end()) return Q3_META_MISSING;
    const Q3GgufMeta& m = it->second;
    if (!is_int_type(m.type)) return Q3_META_TYPE;
    const uint64_t u = load_int((const uint8_t*)map_ + m.off, m.type);
    if (m.type == Q3_GV_U64 && u > (uint64_t)INT64_MAX) return Q3_META_TYPE;
    *v = (int64_t)u;
    return Q3_META_OK;
}
int Q3Gguf::meta_float(const std::string& key, double* v) const {
    auto it = meta_.find(key);
    if (it == meta_.end()) return Q3_META_MISSING;
    if (!is_float_type(it->second.type)) return Q3_META_TYPE;
    *v = load_float((const uint8_t*)map_ + it->second.off, it->second.type);
    return Q3_META_OK;
}
int Q3Gguf::meta_str(const std::string& key, std::string* v) const {
    auto it = meta_.find(key);
    if (it == meta_.end()) return Q3_META_MISSING;
    if (it->second.type != Q3_GV_STR) return Q3_META_TYPE;
    v->assign((const char*)map_ + it->second.off, it->second.end - it->second.off);
    return Q3_META_OK;
}
int Q3Gguf::meta_int_array(const std::string& key, std::vector<int64_t>* v) const {
    auto it = meta_.find(key);
    if (it == meta_.end()) return Q3_META_MISSING;
    const Q3GgufMeta& m = it->second;
    if (m.type != Q3_GV_ARR || !is_int_type(m.elem_type)) return Q3_META_TYPE;
    const size_t es = scalar_size(m.elem_type);
    v->resize((size_t)m.count);
    for (size_t j = 0; j < (size_t)m.count; ++j) {
        const uint64_t u = load_int((const uint8_t*)map_ + m.off + j * es, m.elem_type);
        if (m.elem_type == Q3_GV_U64 && u > (uint64_t)INT64_MAX) return Q3_META_TYPE;
        (*v)[j] = (int64_t)u;
    }
    return Q3_META_OK;
}
int Q3Gguf::meta_float_array(const std::string& key, std::vector<double>* v) const {
    auto it = meta_.find(key);
    if (it == meta_.end()) return Q3_META_MISSING;
    const Q3GgufMeta& m = it->second;
    if (m.type != Q3_GV_ARR || !is_float_type(m.elem_type)) return Q3_META_TYPE;
    const size_t es = scalar_size(m.elem_type);
    v->resize((size_t)m.count);
    for (size_t j = 0; j < (size_t)m.count; ++j) (*v)[j] = load_float((const uint8_t*)map_ + m.off + j * es, m.elem_type);
    return Q3_META_OK;
}

int q3_gguf_to_f32(const Q3GgufTensor& t, float* dst, std::string& err) {
    if (!t.data) { err = "tensor '" + t.name + "': unsupported ggml type " + std::to_string(t.type) + " (supported: F32, F16, BF16, Q8_0, Q4_K, Q5_K, Q6_K)"; return -1; }
    const size_t n = t.nelem;
    if (t.type == Q3_GGML_Q4_K || t.type == Q3_GGML_Q5_K || t.type == Q3_GGML_Q6_K) { for (size_t kb = 0; kb < n / 256; ++kb) deq_k_block(t, kb, dst + kb * 256); return 0; }
    if (t.type == Q3_GGML_F32) memcpy(dst, t.data, n * 4);
    else if (t.type == Q3_GGML_F16) { for (size_t i = 0; i < n; ++i) { uint16_t h; memcpy(&h, t.data + 2 * i, 2); dst[i] = f16_to_f32(h); } }
    else if (t.type == Q3_GGML_BF16) { for (size_t i = 0; i < n; ++i) { uint16_t h; memcpy(&h, t.data + 2 * i, 2); const uint32_t u = (uint32_t)h << 16; memcpy(&dst[i], &u, 4); } }
    else {  // Q8_0: blocks of { f16 d; int8 q[32] }, y = q * f32(d)
        for (size_t b = 0; b < n / 32; ++b) {
            const uint8_t* blk = t.data + b * 34;
            uint16_t h; memcpy(&h, blk, 2);
            const float d = f16_to_f32(h);
            for (int j = 0; j < 32; ++j) dst[b * 32 + j] = (float)(int8_t)blk[2 + j] * d;
        }
    }
    return 0;
}

int q3_gguf_to_bf16(const Q3GgufTensor& t, uint16_t* dst, std::string& err) {
    if (!t.data) { err = "tensor '" + t.name + "': unsupported ggml type " + std::to_string(t.type) + " (supported: F32, F16, BF16, Q8_0, Q4_K, Q5_K, Q6_K)"; return -1; }
    if (t.type == Q3_GGML_BF16) { memcpy(dst, t.data, t.nelem * 2); return 0; }
    if (t.type == Q3_GGML_Q4_K || t.type == Q3_GGML_Q5_K || t.type == Q3_GGML_Q6_K) {
        float y[256];
        for (size_t kb = 0; kb < t.nelem / 256; ++kb) { deq_k_block(t, kb, y); for (int j = 0; j < 256; ++j) dst[kb * 256 + j] = f32_to_bf16_rne(y[j]); }
        return 0;
    }
    const size_t chunk = 1 << 16;
    std::vector<float> tmp(chunk);
    if (t.type == Q3_GGML_F32) {
        for (size_t i = 0; i < t.nelem; ++i) { float f; memcpy(&f, t.data + 4 * i, 4); dst[i] = f32_to_bf16_rne(f); }
    } else if (t.type == Q3_GGML_F16) {
        for (size_t i = 0; i < t.nelem; ++i) { uint16_t h; memcpy(&h, t.data + 2 * i, 2); dst[i] = f32_to_bf16_rne(f16_to_f32(h)); }
    } else {
        for (size_t b = 0; b < t.nelem / 32; ++b) {
            const uint8_t* blk = t.data + b * 34;
            uint16_t h; memcpy(&h, blk, 2);
            const float d = f16_to_f32(h);
            for (int j = 0; j < 32; ++j) dst[b * 32 + j] = f32_to_bf16_rne((float)(int8_t)blk[2 + j] * d);
        }
    }
    return 0;
}

// header of an NPY v1/v2 file holding little-endian f32 in C order: the shape; *fp stays open at the first data byte
static int npy_open(const std::string& path, FILE** fp, std::vector<size_t>& shape, std::string& err) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { err = "cannot open " + path; return -1; }
    unsigned char magic[10];
    if (fread(magic, 1, 10, f) != 10 || memcmp(magic, "\x93NUMPY", 6) != 0) { fclose(f); err = path + ": not a numpy file"; return -1; }
    size_t hlen = 0;
    if (magic[6] == 1) hlen = (size_t)magic[8] | ((size_t)magic[9] << 8);
    else if (magic[6] == 2) {
        unsigned char more[2];
        if (fread(more, 1, 2, f) != 2) { fclose(f); err = path + ": truncated header"; return -1; }
        hlen = (size_t)magic[8] | ((size_t)magic[9] << 8) | ((size_t)more[0] << 16) | ((size_t)more[1] << 24);
    } else { fclose(f); err = path + ": unsupported numpy version"; return -1; }
    if (hlen > (1u << 20)) { fclose(f); err = path + ": header too long"; return -1; }
    std::string header(hlen, '\0');
    if (fread(&header[0], 1, hlen, f) != hlen) { fclose(f); err = path + ": truncated header"; return -1; }
    if (header.find("'<f4'") == std::string::npos && header.find("\"<f4\"") == std::string::npos) { fclose(f); err = path + ": dtype is not little-endian f32"; return -1; }
    if (header.find("'fortran_order': True") != std::string::npos) { fclose(f); err = path + ": fortran_order arrays are not supported"; return -1; }
    shape.clear();
    const size_t sp = header.find("shape");
    const size_t lp = sp == std::string::npos ? std::string::npos : header.find('(', sp), rp = lp == std::string::npos ? std::string::npos : header.find(')', lp);
    if (rp == std::string::npos) { fclose(f); err = path + ": no shape in header"; return -1; }
    size_t v = 0; bool have = false;
    for (size_t i = lp + 1; i <= rp; ++i) {
        const char ch = header[i];
        if (ch >= '0' && ch <= '9') { v = v * 10 + (size_t)(ch - '0'); have = true; }
        else { if (have) shape.push_back(v); v = 0; have = false; }
    }
    *fp = f;
    return 0;
}

int q3_npy_load_f32(const std::string& path, std::vector<float>& out, std::vector<size_t>& shape, std::string& err) {
    FILE* f = nullptr;
    if (npy_open(path, &f, shape, err)) return -1;
    size_t n = 1;
    for (size_t d : shape) n *= d;
    out.resize(n);
    if (n && fread(out.data(), 4, n, f) != n) { fclose(f); err = path + ": truncated data"; return -1; }
    fclose(f);
    return 0;
}

int q3_npy_shape(const std::string& path, std::vector<size_t>& shape, std::string& err) {
    FILE* f = nullptr;
    if (npy_open(path, &f, shape, err)) return -1;
    fclose(f);
    return 0;
}

// ---- the vocoder's weights file (q3_gguf.h; the table is DESIGN.md §27) ----------------------------------------------------------------
#include "../../include/q3tts.h"

#include <algorithm>
#include <cmath>
#include <set>

namespace {

const char* const kVocArch = "q3tts-vocoder";

// how a file tensor (PyTorch layout) becomes the device's array
enum VfKind {
    VF_COPY,     // vectors, [out][in] matrices, codebook tables: as stored
    VF_CONV,     // Conv1d [n][ci][k] -> W[tap][n][ci]
    VF_CONVT,    // ConvTranspose1d [i][o][r] (kernel = stride = r) -> W[j][o][i]
    VF_CONVT2,   // ConvTranspose1d [i][o][2r] (stride r) -> W[tap][j][o][i]: tap 1 = kernel taps 0 .. r-1 (the current step), tap 0 = r .. 2r-1
    VF_DW,       // depth-wise Conv1d [c][1][7] -> [7][c]
    VF_SNAKE_A,  // log alpha -> exp(alpha)
    VF_SNAKE_B   // log beta -> 1 / (exp(beta) + 1e-9)
};
struct VfSpec { std::string name; std::vector<int64_t> shape; VfKind kind = VF_COPY; bool bf16 = false; };

// decoder block b's input channels
int64_t vf_block_in(const q3tts_vocoder_config& c, int b) { int64_t ch = c.decoder_dim; for (int i = 0; i < b; ++i) ch /= 2; return ch; }

// generator id (comp, which) -> file tensor; false for an id the shape vc does not have
bool vf_spec(const q3tts_vocoder_config& c, int comp, int which, VfSpec* s) {
    const int64_t d = c.latent_dim, H = (int64_t)c.n_head * c.head_dim, F = c.d_ffn, dd = c.decoder_dim;
    auto set = [&](const std::string& name, std::vector<int64_t> shape, VfKind kind, bool bf16) { s->name = name; s->shape = std::move(shape); s->kind = kind; s->bf16 = bf16; return true; };
    auto vec = [&](const std::string& name, int64_t n) { return set(name, {n}, VF_COPY, false); };
    auto mat = [&](const std::string& name, int64_t rows, int64_t cols) { return set(name, {rows, cols}, VF_COPY, true); };
    auto conv = [&](const std::string& name, int64_t n, int64_t ci, int64_t k) { return set(name, {n, ci, k}, VF_CONV, true); };
    if (comp >= VC_CODEBOOK && comp < VC_CODEBOOK + c.n_codebooks && comp < VC_PRE)
        return which == VW_W && mat("codebook." + std::to_string(comp - VC_CODEBOOK) + ".weight", c.codebook_size, c.codebook_dim);
    if (comp == VC_PRE) {
        if (which == VW_W) return conv("pre_conv.conv.weight", d, c.codebook_dim, c.pre_conv_kernel);
        return which == VW_B && vec("pre_conv.conv.bias", d);
    }
    if (comp >= VC_TFM && comp < VC_TFM + c.n_layer && comp < VC_FINAL_NORM) {
        const std::string p = "pre_transformer.layers." + std::to_string(comp - VC_TFM) + ".";
        switch (which) {
            case VW_IN_NORM: return vec(p + "input_layernorm.weight", d);
            case VW_POST_NORM: return vec(p + "post_attention_layernorm.weight", d);
            case VW_LS_ATTN: return vec(p + "self_attn_layer_scale.scale", d);
            case VW_LS_MLP: return vec(p + "mlp_layer_scale.scale", d);
            case VW_Q: return mat(p + "self_attn.q_proj.weight", H, d);
            case VW_K: return mat(p + "self_attn.k_proj.weight", H, d);
            case VW_V: return mat(p + "self_attn.v_proj.weight", H, d);
            case VW_O: return mat(p + "self_attn.o_proj.weight", d, H);
            case VW_GATE: return mat(p + "mlp.gate_proj.weight", F, d);
            case VW_UP: return mat(p + "mlp.up_proj.weight", F, d);
            case VW_DOWN: return mat(p + "mlp.down_proj.weight", d, F);
            default: return false;
        }
    }
    if (comp == VC_FINAL_NORM) return which == VW_W && vec("pre_transformer.norm.weight", d);
    if (comp >= VC_UP && comp < VC_UP + c.n_upsample && comp < VC_UP + Q3TTS_MAX_UPSAMPLE) {
        const int u = comp - VC_UP;
        const std::string p = "upsample." + std::to_string(u) + ".";
        switch (which) {
            case VW_W: return set(p + "0.conv.weight", {d, d, c.upsample_ratios[u]}, VF_CONVT, true);
            case VW_B: return vec(p + "0.conv.bias", d);
            case VW_DW_W: return set(p + "1.dwconv.conv.weight", {d, 1, 7}, VF_DW, false);
            case VW_DW_B: return vec(p + "1.dwconv.conv.bias", d);
            case VW_LN_W: return vec(p + "1.norm.weight", d);
            case VW_LN_B: return vec(p + "1.norm.bias", d);
            case VW_PW1: return mat(p + "1.pwconv1.weight", 4 * d, d);
            case VW_PW1_B: return vec(p + "1.pwconv1.bias", 4 * d);
            case VW_PW2: return mat(p + "1.pwconv2.weight", d, 4 * d);
            case VW_PW2_B: return vec(p + "1.pwconv2.bias", d);
            case VW_GAMMA: return vec(p + "1.gamma", d);
            default: return false;
        }
    }
    if (comp == VC_DEC_IN) {
        if (which == VW_W) return conv("decoder.0.conv.weight", dd, d, 7);
        return which == VW_B && vec("decoder.0.conv.bias", dd);
    }
    if (comp >= VC_BLK && comp < VC_BLK + 4 * c.n_dec_blocks && comp < VC_BLK + 4 * Q3TTS_MAX_DEC_BLOCKS) {
        const int b = (comp - VC_BLK) / 4, part = (comp - VC_BLK) % 4;
        const int64_t ch = vf_block_in(c, b), co = ch / 2, r = c.dec_rates[b];
        const std::string p = "decoder." + std::to_string(1 + b) + ".block.";
        if (part == 0) switch (which) {
            case VW_ALPHA: return set(p + "0.alpha", {ch}, VF_SNAKE_A, false);
            case VW_BETA: return set(p + "0.beta", {ch}, VF_SNAKE_B, false);
            case VW_W: return set(p + "1.conv.weight", {ch, co, 2 * r}, VF_CONVT2, true);
            case VW_B: return vec(p + "1.conv.bias", co);
            default: return false;
        }
        const std::string q = p + std::to_string(1 + part) + ".";
        switch (which) {
            case VW_ALPHA: return set(q + "act1.alpha", {co}, VF_SNAKE_A, false);
            case VW_BETA: return set(q + "act1.beta", {co}, VF_SNAKE_B, false);
            case VW_W: return conv(q + "conv1.conv.weight", co, co, 7);
            case VW_B: return vec(q + "conv1.conv.bias", co);
            case VW_ALPHA2: return set(q + "act2.alpha", {co}, VF_SNAKE_A, false);
            case VW_BETA2: return set(q + "act2.beta", {co}, VF_SNAKE_B, false);
            case VW_W2: return conv(q + "conv2.conv.weight", co, co, 1);
            case VW_B2: return vec(q + "conv2.conv.bias", co);
            default: return false;
        }
    }
    if (comp == VC_OUT) {
        const int64_t ch = vf_block_in(c, c.n_dec_blocks);
        switch (which) {
            case VW_ALPHA: return set("decoder." + std::to_string(1 + c.n_dec_blocks) + ".alpha", {ch}, VF_SNAKE_A, false);
            case VW_BETA: return set("decoder." + std::to_string(1 + c.n_dec_blocks) + ".beta", {ch}, VF_SNAKE_B, false);
            case VW_W: return conv("decoder." + std::to_string(2 + c.n_dec_blocks) + ".conv.weight", 1, ch, 7);
            case VW_B: return vec("decoder." + std::to_string(2 + c.n_dec_blocks) + ".conv.bias", 1);
            default: return false;
        }
    }
    return false;
}

// every id the shape vc has, in the order q3_voc_create takes them
std::vector<std::pair<int, int>> vf_ids(const q3tts_vocoder_config& c) {
    std::vector<std::pair<int, int>> ids;
    for (int q = 0; q < c.n_codebooks; ++q) ids.push_back({VC_CODEBOOK + q, VW_W});
    ids.push_back({VC_PRE, VW_W}); ids.push_back({VC_PRE, VW_B});
    for (int l = 0; l < c.n_layer; ++l)
        for (int w : {VW_IN_NORM, VW_POST_NORM, VW_LS_ATTN, VW_LS_MLP, VW_Q, VW_K, VW_V, VW_O, VW_GATE, VW_UP, VW_DOWN}) ids.push_back({VC_TFM + l, w});
    ids.push_back({VC_FINAL_NORM, VW_W});
    for (int u = 0; u < c.n_upsample; ++u)
        for (int w : {VW_W, VW_B, VW_DW_W, VW_DW_B, VW_LN_W, VW_LN_B, VW_PW1, VW_PW1_B, VW_PW2, VW_PW2_B, VW_GAMMA}) ids.push_back({VC_UP + u, w});
    ids.push_back({VC_DEC_IN, VW_W}); ids.push_back({VC_DEC_IN, VW_B});
    for (int b = 0; b < c.n_dec_blocks; ++b) {
        for (int w : {VW_ALPHA, VW_BETA, VW_W, VW_B}) ids.push_back({VC_BLK + 4 * b, w});
        for (int u = 1; u <= 3; ++u)
            for (int w : {VW_ALPHA, VW_BETA, VW_W, VW_B, VW_ALPHA2, VW_BETA2, VW_W2, VW_B2}) ids.push_back({VC_BLK + 4 * b + u, w});
    }
    for (int w : {VW_ALPHA, VW_BETA, VW_W, VW_B}) ids.push_back({VC_OUT, w});
    return ids;
}

std::string vf_shape_str(const std::vector<int64_t>& s) { std::string r; for (int64_t v : s) r += "[" + std::to_string(v) + "]"; return r; }

// the file's tensor of `s`, present and of its PyTorch shape (GGUF lists dimensions innermost first); `whence` says where the expected shape came from
const Q3GgufTensor* vf_tensor(const Q3Gguf& g, const std::string& file, const VfSpec& s, const char* whence, std::string& err) {
    const Q3GgufTensor* t = g.find(s.name);
    if (!t) { err = file + ": tensor '" + s.name + "' is missing"; return nullptr; }
    std::vector<int64_t> have(t->dims.rbegin(), t->dims.rend());
    if (have != s.shape) { err = file + ": tensor '" + s.name + "' has shape " + vf_shape_str(have) + ", " + whence + " " + vf_shape_str(s.shape); return nullptr; }
    return t;
}

// the metadata: every key is required
struct VfIntKey { const char* key; int32_t q3tts_vocoder_config::*field; };
const VfIntKey kVfInts[] = {
    {"n_codebooks", &q3tts_vocoder_config::n_codebooks}, {"codebook_size", &q3tts_vocoder_config::codebook_size},
    {"codebook_dim", &q3tts_vocoder_config::codebook_dim}, {"latent_dim", &q3tts_vocoder_config::latent_dim},
    {"pre_conv_kernel", &q3tts_vocoder_config::pre_conv_kernel}, {"block_count", &q3tts_vocoder_config::n_layer},
    {"attention.head_count", &q3tts_vocoder_config::n_head}, {"attention.key_length", &q3tts_vocoder_config::head_dim},
    {"feed_forward_length", &q3tts_vocoder_config::d_ffn}, {"attention.sliding_window", &q3tts_vocoder_config::sliding_window},
    {"decoder_dim", &q3tts_vocoder_config::decoder_dim}, {"sample_rate", &q3tts_vocoder_config::sample_rate},
};
std::string vf_key(const char* k) { return std::string(kVocArch) + "." + k; }

int vf_read_meta(const Q3Gguf& g, const std::string& file, q3tts_vocoder_config* vc, std::string& err) {
    auto bad = [&](const std::string& m) { err = file + ": " + m; return -1; };
    std::string arch;
    const int st = g.meta_str("general.architecture", &arch);
    if (st == Q3_META_MISSING) return bad("metadata key 'general.architecture' is missing");
    if (st == Q3_META_TYPE) return bad("metadata key 'general.architecture' is not a string");
    if (arch != kVocArch) return bad("metadata key 'general.architecture' = '" + arch + "', a vocoder file has '" + kVocArch + "'");
    auto integer = [&](const std::string& k, int64_t lo, int32_t* out) {
        int64_t v = 0;
        const int s = g.meta_int(k, &v);
        if (s == Q3_META_MISSING) return bad("metadata key '" + k + "' is missing");
        if (s == Q3_META_TYPE) return bad("metadata key '" + k + "' is not an integer");
        if (v < lo || v > (1 << 24)) return bad("metadata key '" + k + "' = " + std::to_string(v) + " is out of range");
        *out = (int32_t)v;
        return 0;
    };
    for (const VfIntKey& k : kVfInts) if (integer(vf_key(k.key), 1, &(vc->*k.field))) return -1;
    if (integer(vf_key("lookahead_frames"), 0, &vc->lookahead_frames)) return -1;
    auto real = [&](const std::string& k, float* out) {
        double v = 0;
        const int s = g.meta_float(k, &v);
        if (s == Q3_META_MISSING) return bad("metadata key '" + k + "' is missing");
        if (s == Q3_META_TYPE) return bad("metadata key '" + k + "' is not a float");
        if (!std::isfinite(v)) return bad("metadata key '" + k + "' is not finite");
        *out = (float)v;
        return 0;
    };
    if (real(vf_key("rope.freq_base"), &vc->rope_theta) || real(vf_key("attention.layer_norm_rms_epsilon"), &vc->rms_eps)) return -1;
    auto ints = [&](const std::string& k, int cap, int32_t* n, int32_t* out) {
        std::vector<int64_t> v;
        const int s = g.meta_int_array(k, &v);
        if (s == Q3_META_MISSING) return bad("metadata key '" + k + "' is missing");
        if (s == Q3_META_TYPE) return bad("metadata key '" + k + "' is not an integer array");
        if ((int64_t)v.size() > cap) return bad("metadata key '" + k + "' has " + std::to_string(v.size()) + " entries, at most " + std::to_string(cap) + " are allowed");
        for (int i = 0; i < cap; ++i) out[i] = 0;
        for (size_t i = 0; i < v.size(); ++i) {
            if (v[i] < 1 || v[i] > 4096) return bad("metadata key '" + k + "' entry " + std::to_string(i) + " = " + std::to_string(v[i]) + " is out of range");
            out[i] = (int32_t)v[i];
        }
        *n = (int32_t)v.size();
        return 0;
    };
    if (ints(vf_key("upsample_ratios"), Q3TTS_MAX_UPSAMPLE, &vc->n_upsample, vc->upsample_ratios)) return -1;
    if (ints(vf_key("decoder_rates"), Q3TTS_MAX_DEC_BLOCKS, &vc->n_dec_blocks, vc->dec_rates)) return -1;
    return 0;
}

// how many distinct N have a tensor "<prefix>N<suffix>..."
int64_t vf_count(const Q3Gguf& g, const std::string& prefix, const std::string& suffix) {
    std::set<std::string> idx;
    for (const Q3GgufTensor& t : g.tensors()) {
        if (t.name.compare(0, prefix.size(), prefix) != 0) continue;
        size_t i = prefix.size();
        while (i < t.name.size() && t.name[i] >= '0' && t.name[i] <= '9') ++i;
        if (i > prefix.size() && t.name.compare(i, suffix.size(), suffix) == 0) idx.insert(t.name.substr(prefix.size(), i - prefix.size()));
    }
    return (int64_t)idx.size();
}

// one tensor as the device's array (see q3_voc_file_array); tmp is scratch
int vf_array(const Q3GgufTensor& t, const VfSpec& s, std::vector<float>& tmp, std::vector<float>& out, std::string& err) {
    const size_t n = t.nelem;
    out.resize(n);
    std::vector<float>& src = s.kind == VF_COPY ? out : tmp;
    src.resize(n);
    if (q3_gguf_to_f32(t, src.data(), err)) return -1;
    const float* w = src.data();
    switch (s.kind) {
        case VF_COPY: break;
        case VF_CONV: {
            const size_t N = (size_t)s.shape[0], CI = (size_t)s.shape[1], K = (size_t)s.shape[2];
            for (size_t nn = 0; nn < N; ++nn) for (size_t ci = 0; ci < CI; ++ci) for (size_t k = 0; k < K; ++k) out[(k * N + nn) * CI + ci] = w[(nn * CI + ci) * K + k];
            break;
        }
        case VF_CONVT: {
            const size_t I = (size_t)s.shape[0], O = (size_t)s.shape[1], R = (size_t)s.shape[2];
            for (size_t i = 0; i < I; ++i) for (size_t o = 0; o < O; ++o) for (size_t j = 0; j < R; ++j) out[(j * O + o) * I + i] = w[(i * O + o) * R + j];
            break;
        }
        case VF_CONVT2: {
            const size_t I = (size_t)s.shape[0], O = (size_t)s.shape[1], R = (size_t)s.shape[2] / 2;
            for (size_t i = 0; i < I; ++i) for (size_t o = 0; o < O; ++o) for (size_t j = 0; j < R; ++j) {
                out[(((size_t)1 * R + j) * O + o) * I + i] = w[(i * O + o) * 2 * R + j];
                out[(((size_t)0 * R + j) * O + o) * I + i] = w[(i * O + o) * 2 * R + R + j];
            }
            break;
        }
        case VF_DW: {
            const size_t C = (size_t)s.shape[0], K = (size_t)s.shape[2];
            for (size_t c = 0; c < C; ++c) for (size_t k = 0; k < K; ++k) out[k * C + c] = w[c * K + k];
            break;
        }
        case VF_SNAKE_A: for (size_t i = 0; i < n; ++i) out[i] = (float)exp((double)w[i]); break;
        case VF_SNAKE_B: for (size_t i = 0; i < n; ++i) out[i] = (float)(1.0 / (exp((double)w[i]) + 1e-9)); break;
    }
    if (s.bf16)
        for (size_t i = 0; i < n; ++i) { const uint32_t u = (uint32_t)f32_to_bf16_rne(out[i]) << 16; memcpy(&out[i], &u, 4); }
    return 0;
}

// every tensor of the shape vc: present, of vc's shape, of a type the reader reads
int vf_check_tensors(const Q3Gguf& g, const std::string& file, const q3tts_vocoder_config& vc, const char* whence, std::string& err) {
    if (vc.n_layer > VC_FINAL_NORM - VC_TFM) { err = file + ": metadata key '" + vf_key("block_count") + "' = " + std::to_string(vc.n_layer) + " is out of range"; return -1; }
    for (const auto& id : vf_ids(vc)) {
        VfSpec s;
        if (!vf_spec(vc, id.first, id.second, &s)) { err = file + ": no tensor for id (" + std::to_string(id.first) + ", " + std::to_string(id.second) + ")"; return -1; }
        const Q3GgufTensor* t = vf_tensor(g, file, s, whence, err);
        if (!t) return -1;
        if (!t->data) { err = file + ": tensor '" + s.name + "': unsupported ggml type " + std::to_string(t->type) + " (supported: F32, F16, BF16, Q8_0, Q4_K, Q5_K, Q6_K)"; return -1; }
    }
    return 0;
}

}  // namespace

// wdir/name (the quant directory), else the same name in wdir's parent (the model directory); "" when neither exists
static std::string file_beside_model(const std::string& wdir, const char* name) {
    auto is_file = [](const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); };
    std::string d = wdir;
    while (d.size() > 1 && d.back() == '/') d.pop_back();
    if (is_file(d + "/" + name)) return d + "/" + name;
    const size_t sl = d.rfind('/');
    const std::string parent = sl == std::string::npos ? std::string(".") : sl == 0 ? std::string("/") : d.substr(0, sl);
    const std::string p = (parent == "/" ? std::string() : parent) + "/" + name;
    return is_file(p) ? p : std::string();
}
std::string q3_voc_file_find(const std::string& wdir) { return file_beside_model(wdir, Q3_VOC_FILE_NAME); }

int q3_voc_file_config(const Q3Gguf& g, const std::string& file, q3tts_vocoder_config* vc, std::string& err) {
    q3tts_vocoder_config c = *vc;  // (*vc is written only on success; layer_scale_init is no file's to state)
    if (vf_read_meta(g, file, &c, err)) return -1;
    auto count = [&](const char* key, int64_t want, const std::string& prefix, const std::string& suffix) {
        const int64_t have = vf_count(g, prefix, suffix);
        if (have == want) return 0;
        err = file + ": metadata key '" + vf_key(key) + "' implies " + std::to_string(want) + " tensors '" + prefix + "N" + suffix + "...', the file has " + std::to_string(have);
        return -1;
    };
    if (count("n_codebooks", c.n_codebooks, "codebook.", ".weight") || count("block_count", c.n_layer, "pre_transformer.layers.", ".") ||
        count("upsample_ratios", c.n_upsample, "upsample.", ".0.conv.weight") || count("decoder_rates", c.n_dec_blocks, "decoder.", ".block.0.alpha")) return -1;
    {   // the decoder halves its channels block by block
        int64_t ch = c.decoder_dim;
        for (int b = 0; b < c.n_dec_blocks; ++b) {
            if (ch % 2) { err = file + ": metadata key '" + vf_key("decoder_dim") + "' = " + std::to_string(c.decoder_dim) + " cannot be halved " + std::to_string(c.n_dec_blocks) + " times ('" + vf_key("decoder_rates") + "')"; return -1; }
            ch /= 2;
        }
    }
    if (vf_check_tensors(g, file, c, "the file's metadata implies", err)) return -1;
    *vc = c;
    return 0;
}

int q3_voc_file_check(const Q3Gguf& g, const std::string& file, const q3tts_vocoder_config& vc, std::string& err) {
    q3tts_vocoder_config m = vc;
    if (vf_read_meta(g, file, &m, err)) return -1;
    auto differs = [&](const std::string& key, const std::string& have, const std::string& want) {
        err = file + ": metadata key '" + key + "' = " + have + ", the configuration has " + want;
        return -1;
    };
    for (const VfIntKey& k : kVfInts) if (m.*k.field != vc.*k.field) return differs(vf_key(k.key), std::to_string(m.*k.field), std::to_string(vc.*k.field));
    if (m.lookahead_frames != vc.lookahead_frames) return differs(vf_key("lookahead_frames"), std::to_string(m.lookahead_frames), std::to_string(vc.lookahead_frames));
    auto g9 = [](float v) { char b[40]; snprintf(b, sizeof b, "%.9g", (double)v); return std::string(b); };
    if (m.rope_theta != vc.rope_theta) return differs(vf_key("rope.freq_base"), g9(m.rope_theta), g9(vc.rope_theta));
    if (m.rms_eps != vc.rms_eps) return differs(vf_key("attention.layer_norm_rms_epsilon"), g9(m.rms_eps), g9(vc.rms_eps));
    auto list = [](const int32_t* v, int n) { std::string r = "["; for (int i = 0; i < n; ++i) r += (i ? ", " : "") + std::to_string(v[i]); return r + "]"; };
    if (m.n_upsample != vc.n_upsample || memcmp(m.upsample_ratios, vc.upsample_ratios, sizeof(int32_t) * (size_t)std::max(0, std::min<int>(vc.n_upsample, Q3TTS_MAX_UPSAMPLE))))
        return differs(vf_key("upsample_ratios"), list(m.upsample_ratios, m.n_upsample), list(vc.upsample_ratios, std::max(0, std::min<int>(vc.n_upsample, Q3TTS_MAX_UPSAMPLE))));
    if (m.n_dec_blocks != vc.n_dec_blocks || memcmp(m.dec_rates, vc.dec_rates, sizeof(int32_t) * (size_t)std::max(0, std::min<int>(vc.n_dec_blocks, Q3TTS_MAX_DEC_BLOCKS))))
        return differs(vf_key("decoder_rates"), list(m.dec_rates, m.n_dec_blocks), list(vc.dec_rates, std::max(0, std::min<int>(vc.n_dec_blocks, Q3TTS_MAX_DEC_BLOCKS))));
    if (vf_check_tensors(g, file, vc, "the configuration needs", err)) return -1;
    std::vector<float> buf;
    for (const auto& id : vf_ids(vc)) {
        VfSpec s;
        vf_spec(vc, id.first, id.second, &s);
        const Q3GgufTensor* t = g.find(s.name);
        buf.resize(t->nelem);
        if (q3_gguf_to_f32(*t, buf.data(), err)) { err = file + ": " + err; return -1; }
        for (size_t i = 0; i < buf.size(); ++i)
            if (!std::isfinite(buf[i])) { err = file + ": tensor '" + s.name + "' holds a value that is not finite (element " + std::to_string(i) + ")"; return -1; }
    }
    return 0;
}

int q3_voc_file_array(const Q3Gguf& g, const std::string& file, const q3tts_vocoder_config& vc, int comp, int which, std::vector<float>& out, std::string& err) {
    VfSpec s;
    if (!vf_spec(vc, comp, which, &s)) { err = file + ": the vocoder shape has no tensor of id (" + std::to_string(comp) + ", " + std::to_string(which) + ")"; return -1; }
    const Q3GgufTensor* t = vf_tensor(g, file, s, "the configuration needs", err);
    if (!t) return -1;
    std::vector<float> tmp;
    if (vf_array(*t, s, tmp, out, err)) { err = file + ": " + err; return -1; }
    return 0;
}

// ---- C ABI test hook (host only) -------------------------------------------------------------------------------
struct q3tts_engine;
int q3_set_err(q3tts_engine* e, int code, const std::string& msg);  // q3_engine.hip (engine == nullptr: the global error slot)

extern "C" int q3tts_vocoder_config_from_file(const char* path, q3tts_vocoder_config* vc, char* err, int32_t err_cap) {
    std::string msg;
    auto done = [&](int rc) {
        if (err && err_cap > 0) { const size_t n = msg.size() < (size_t)err_cap - 1 ? msg.size() : (size_t)err_cap - 1; memcpy(err, msg.data(), n); err[n] = '\0'; }
        return rc;
    };
    if (!path || !vc) { msg = "null argument"; return done(Q3TTS_ERR_INVALID); }
    Q3Gguf g;
    if (g.open(path, msg)) return done(Q3TTS_ERR_IO);
    return done(q3_voc_file_config(g, path, vc, msg) ? Q3TTS_ERR_INVALID : Q3TTS_OK);
}

extern "C" int q3tts_k_voc_file_tensor(const char* path, const q3tts_vocoder_config* vc, int32_t comp, int32_t which, float* out, int64_t cap, int64_t* n) {
    if (!path || !vc || !n) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    std::string err;
    Q3Gguf g;
    if (g.open(path, err)) return q3_set_err(nullptr, Q3TTS_ERR_IO, err);
    std::vector<float> a;
    if (q3_voc_file_array(g, path, *vc, comp, which, a, err)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, err);
    *n = (int64_t)a.size();
    if (out) {
        if (cap < *n) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "output buffer too small");
        memcpy(out, a.data(), a.size() * 4);
    }
    return Q3TTS_OK;
}

extern "C" int q3tts_k_gguf_read(const char* path, const char* tensor, float* out, int64_t cap, int64_t* nelem, int64_t* dims4, int32_t* ggml_type) {
    if (!path || !tensor || !nelem) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    std::string err;
    const std::string p = path;
    if (p.size() > 4 && p.compare(p.size() - 4, 4, ".npy") == 0) {
        std::vector<float> v; std::vector<size_t> shape;
        if (q3_npy_load_f32(p, v, shape, err)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, err);
        *nelem = (int64_t)v.size();
        if (dims4) for (int i = 0; i < 4; ++i) dims4[i] = i < (int)shape.size() ? (int64_t)shape[i] : 0;
        if (ggml_type) *ggml_type = Q3_GGML_F32;
        if (out) { if (cap < *nelem) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "output buffer too small"); memcpy(out, v.data(), v.size() * 4); }
        return Q3TTS_OK;
    }
    Q3Gguf g;
    if (g.open(p, err)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, err);
    const Q3GgufTensor* t = g.find(tensor);
    if (!t) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, std::string("tensor '") + tensor + "' is missing");
    *nelem = (int64_t)t->nelem;
    if (dims4) for (int i = 0; i < 4; ++i) dims4[i] = i < (int)t->dims.size() ? (int64_t)t->dims[i] : 0;
    if (ggml_type) *ggml_type = (int32_t)t->type;
    if (out) {
        if (cap < *nelem) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "output buffer too small");
        if (q3_gguf_to_f32(*t, out, err)) return q3_set_err(nullptr, Q3TTS_ERR_UNSUPPORTED, err);
    }
    return Q3TTS_OK;
}

extern "C" int q3tts_k_gguf_meta(const char* path, const char* key, int32_t* value_type, int32_t* elem_type, int64_t* count, double* values,
                                 int64_t values_cap, char* str, int64_t str_cap, int64_t* str_bytes) {
    if (!path || !key) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    std::string err;
    Q3Gguf g;
    if (g.open(path, err)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, err);
    Q3GgufMeta m;
    if (!g.meta_info(key, &m)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, std::string("metadata key '") + key + "' is missing");
    if (value_type) *value_type = (int32_t)m.type;
    if (elem_type) *elem_type = (int32_t)m.elem_type;
    if (count) *count = (int64_t)m.count;
    size_t nb = 0;
    const uint8_t* raw = g.meta_raw(key, &nb);
    const bool text = m.elem_type == Q3_GV_STR;
    if (str_bytes) *str_bytes = text ? (int64_t)nb : 0;
    if (text) {
        if (str) { if (str_cap < (int64_t)nb) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "string buffer too small"); memcpy(str, raw, nb); }
        return Q3TTS_OK;
    }
    if (values) {
        if (values_cap < (int64_t)m.count) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "value buffer too small");
        const size_t es = scalar_size(m.elem_type);
        for (size_t j = 0; j < (size_t)m.count; ++j) {
            const uint8_t* p = raw + j * es;
            if (is_float_type(m.elem_type)) values[j] = load_float(p, m.elem_type);
            else if (m.elem_type == Q3_GV_U64) values[j] = (double)load_int(p, m.elem_type);
            else values[j] = (double)(int64_t)load_int(p, m.elem_type);
        }
    }
    return Q3TTS_OK;
}

// ---- the clone encoders' weights files (q3_gguf.h; the table is DESIGN.md §29) ---------------------------------------------------------
namespace {

const char* const kSpkArch = "q3tts-speaker-encoder";
const char* const kCodecArch = "q3tts-codec-encoder";

// how the file's tensors (PyTorch layout) become the device's array
enum CfKind {
    CF_VEC,   // biases, LayerNorm, LayerScale: [n] as stored
    CF_BOOK,  // codebook table [codebook_size][vq_dim]: as stored
    CF_CONV,  // Conv1d [n][cin][k] -> rows W[n][tap * cin + ci], zero-padded to kp, bf16
    CF_LIN,   // Linear [n][cin] -> rows W[n][ci], zero-padded to kp, bf16
    CF_QKV    // three Linear [dq][cin] (q, k, v) -> the rows of the first under those of the second under those of the third, as CF_LIN
};
struct CfSpec { int file = 0; std::vector<std::string> names; std::vector<int64_t> shape; CfKind kind = CF_VEC; };  // file: 0 speaker, 1 codec

inline int64_t cf_round512(int64_t k) { return (k + 511) / 512 * 512; }

// generator id (comp, which) -> file tensor(s); false for an id the shape c does not have
bool cf_spec(const q3tts_clone_config& c, int comp, int which, CfSpec* s) {
    auto conv = [&](int file, const std::string& base, int w0, int64_t n, int64_t cin, int64_t k, bool bias) {
        s->file = file;
        if (which == w0) { s->names = {base + ".weight"}; s->shape = {n, cin, k}; s->kind = CF_CONV; return true; }
        if (bias && which == w0 + 1) { s->names = {base + ".bias"}; s->shape = {n}; s->kind = CF_VEC; return true; }
        return false;
    };
    const int64_t C = c.se_channels[0], C4 = c.se_channels[4], S = c.se_res2net_scale > 0 ? c.se_res2net_scale : 1, wp = C / S;
    if (comp == SC_TDNN0) return conv(0, "blocks.0.conv", 0, C, c.mel_dim, c.se_kernels[0], true);
    if (comp >= SC_BLOCK && comp < SC_BLOCK + 3) {
        const int i = comp - SC_BLOCK + 1;
        const std::string p = "blocks." + std::to_string(i) + ".";
        if (which >= SW_RES2 + 2 && which < SW_RES2 + 2 * S) {
            const int br = (which - SW_RES2) / 2;  // branch 1 .. S-1 is the family's blocks[br - 1]
            return conv(0, p + "res2net_block.blocks." + std::to_string(br - 1) + ".conv", SW_RES2 + 2 * br, wp, wp, c.se_kernels[i], true);
        }
        switch (which & ~1) {
            case SW_TDNN1: return conv(0, p + "tdnn1.conv", SW_TDNN1, C, C, 1, true);
            case SW_TDNN2: return conv(0, p + "tdnn2.conv", SW_TDNN2, C, C, 1, true);
            case SW_SE1: return conv(0, p + "se_block.conv1", SW_SE1, c.se_se_channels, C, 1, true);
            case SW_SE2: return conv(0, p + "se_block.conv2", SW_SE2, C, c.se_se_channels, 1, true);
            default: return false;
        }
    }
    if (comp == SC_MFA) return conv(0, "mfa.conv", 0, C4, 3 * C, c.se_kernels[4], true);
    if (comp == SC_ASP_TDNN) return conv(0, "asp.tdnn.conv", 0, c.se_attn_channels, 3 * C4, 1, true);
    if (comp == SC_ASP_CONV) return conv(0, "asp.conv", 0, C4, c.se_attn_channels, 1, true);
    if (comp == SC_FC) return conv(0, "fc", 0, c.se_dim, 2 * C4, 1, true);
    // the audio encoder: SEANet layer indices are the family's (an ELU between the convolutions takes one index each)
    const int nr = c.ae_n_ratios;
    if (comp == AC_CONV0) return conv(1, "encoder.layers.0.conv", 0, c.ae_filters, 1, c.ae_kernel, true);
    if (comp >= AC_STAGE && comp < AC_STAGE + 4 * nr && comp < AC_STAGE + 16) {
        const int i = (comp - AC_STAGE) / 4, part = (comp - AC_STAGE) % 4, li = 1 + 3 * i;
        int64_t Ca = c.ae_filters;
        for (int j = 0; j < i; ++j) Ca *= 2;
        const std::string p = "encoder.layers." + std::to_string(li);
        if (part == 0) return conv(1, p + ".block.1.conv", 0, Ca / 2, Ca, c.ae_res_kernel, true);
        if (part == 1) return conv(1, p + ".block.3.conv", 0, Ca, Ca / 2, 1, true);
        if (part == 2) return conv(1, "encoder.layers." + std::to_string(li + 2) + ".conv", 0, 2 * Ca, Ca, 2 * (int64_t)c.ae_ratios[i], true);
        return false;
    }
    const int64_t H = c.ae_hidden, dq = (int64_t)c.ae_n_head * c.ae_head_dim, F = c.ae_d_ffn;
    if (comp == AC_LAST) {
        int64_t Ca = c.ae_filters;
        for (int j = 0; j < nr; ++j) Ca *= 2;
        return conv(1, "encoder.layers." + std::to_string(3 * nr + 2) + ".conv", 0, H, Ca, c.ae_last_kernel, true);
    }
    if (comp >= AC_TFM && comp < AC_TFM + c.ae_n_layer && comp < AC_DOWN) {
        const std::string p = "encoder_transformer.layers." + std::to_string(comp - AC_TFM) + ".";
        s->file = 1;
        auto vec = [&](const std::string& name) { s->names = {p + name}; s->shape = {H}; s->kind = CF_VEC; return true; };
        auto lin = [&](const std::string& name, int64_t n, int64_t cin) { s->names = {p + name}; s->shape = {n, cin}; s->kind = CF_LIN; return true; };
        switch (which) {
            case TW_LN1_W: return vec("input_layernorm.weight");
            case TW_LN1_B: return vec("input_layernorm.bias");
            case TW_LN2_W: return vec("post_attention_layernorm.weight");
            case TW_LN2_B: return vec("post_attention_layernorm.bias");
            case TW_LS1: return vec("self_attn_layer_scale.scale");
            case TW_LS2: return vec("mlp_layer_scale.scale");
            case TW_QKV:
                s->names = {p + "self_attn.q_proj.weight", p + "self_attn.k_proj.weight", p + "self_attn.v_proj.weight"};
                s->shape = {dq, H}; s->kind = CF_QKV;
                return true;
            case TW_O: return lin("self_attn.o_proj.weight", H, dq);
            case TW_FC1: return lin("mlp.fc1.weight", F, H);
            case TW_FC2: return lin("mlp.fc2.weight", H, F);
            default: return false;
        }
    }
    if (comp == AC_DOWN) return conv(1, "downsample.conv", 0, H, H, 2 * (int64_t)c.ae_down_stride, false);
    if (comp == AC_SEM_PROJ) return conv(1, "quantizer.semantic_residual_vector_quantizer.input_proj", 0, c.ae_vq_dim, H, 1, false);
    if (comp == AC_AC_PROJ) return conv(1, "quantizer.acoustic_residual_vector_quantizer.input_proj", 0, c.ae_vq_dim, H, 1, false);
    if (comp >= AC_CODEBOOK && comp < AC_CODEBOOK + c.ae_n_codebooks && which == 0) {
        s->file = 1; s->names = {"quantizer.codebook." + std::to_string(comp - AC_CODEBOOK) + ".weight"};
        s->shape = {c.ae_codebook_size, c.ae_vq_dim}; s->kind = CF_BOOK;
        return true;
    }
    return false;
}

// every id the shape c has, in the order q3_clone.hip creates them
std::vector<std::pair<int, int>> cf_ids(const q3tts_clone_config& c) {
    std::vector<std::pair<int, int>> ids;
    auto wb = [&](int comp, int w) { ids.push_back({comp, w}); ids.push_back({comp, w + 1}); };
    wb(SC_TDNN0, 0);
    for (int i = 0; i < 3; ++i) {
        wb(SC_BLOCK + i, SW_TDNN1);
        for (int p = 1; p < c.se_res2net_scale; ++p) wb(SC_BLOCK + i, SW_RES2 + 2 * p);
        wb(SC_BLOCK + i, SW_TDNN2); wb(SC_BLOCK + i, SW_SE1); wb(SC_BLOCK + i, SW_SE2);
    }
    wb(SC_MFA, 0); wb(SC_ASP_TDNN, 0); wb(SC_ASP_CONV, 0); wb(SC_FC, 0);
    wb(AC_CONV0, 0);
    for (int i = 0; i < c.ae_n_ratios; ++i) for (int part = 0; part < 3; ++part) wb(AC_STAGE + 4 * i + part, 0);
    wb(AC_LAST, 0);
    for (int l = 0; l < c.ae_n_layer; ++l)
        for (int w : {TW_LN1_W, TW_LN1_B, TW_LN2_W, TW_LN2_B, TW_LS1, TW_LS2, TW_QKV, TW_O, TW_FC1, TW_FC2}) ids.push_back({AC_TFM + l, w});
    ids.push_back({AC_DOWN, 0}); ids.push_back({AC_SEM_PROJ, 0}); ids.push_back({AC_AC_PROJ, 0});
    for (int q = 0; q < c.ae_n_codebooks; ++q) ids.push_back({AC_CODEBOOK + q, 0});
    return ids;
}

const Q3Gguf& cf_gguf(const Q3CloneFiles& f, const CfSpec& s) { return s.file ? f.codec : f.spk; }
const std::string& cf_path(const Q3CloneFiles& f, const CfSpec& s) { return s.file ? f.codec_path : f.spk_path; }

// the file's tensors of `s`: present, of the PyTorch shape, of a type the reader reads
int cf_tensors(const Q3CloneFiles& f, const CfSpec& s, const char* whence, const Q3GgufTensor** out, std::string& err) {
    for (size_t i = 0; i < s.names.size(); ++i) {
        VfSpec v; v.name = s.names[i]; v.shape = s.shape;
        const Q3GgufTensor* t = vf_tensor(cf_gguf(f, s), cf_path(f, s), v, whence, err);
        if (!t) return -1;
        if (!t->data) { err = cf_path(f, s) + ": tensor '" + v.name + "': unsupported ggml type " + std::to_string(t->type) + " (supported: F32, F16, BF16, Q8_0, Q4_K, Q5_K, Q6_K)"; return -1; }
        out[i] = t;
    }
    return 0;
}

struct CfMeta {
    const Q3Gguf& g; const std::string& file; const char* arch; std::string& err;
    int bad(const std::string& m) { err = file + ": " + m; return -1; }
    std::string key(const char* k) const { return std::string(arch) + "." + k; }
    int check_arch() {
        std::string a;
        const int st = g.meta_str("general.architecture", &a);
        if (st == Q3_META_MISSING) return bad("metadata key 'general.architecture' is missing");
        if (st == Q3_META_TYPE) return bad("metadata key 'general.architecture' is not a string");
        if (a != arch) return bad("metadata key 'general.architecture' = '" + a + "', this file has '" + arch + "'");
        return 0;
    }
    int integer(const char* k0, int64_t lo, int32_t* out) {
        const std::string k = key(k0);
        int64_t v = 0;
        const int s = g.meta_int(k, &v);
        if (s == Q3_META_MISSING) return bad("metadata key '" + k + "' is missing");
        if (s == Q3_META_TYPE) return bad("metadata key '" + k + "' is not an integer");
        if (v < lo || v > (1 << 24)) return bad("metadata key '" + k + "' = " + std::to_string(v) + " is out of range");
        *out = (int32_t)v;
        return 0;
    }
    int real(const char* k0, float* out) {
        const std::string k = key(k0);
        double v = 0;
        const int s = g.meta_float(k, &v);
        if (s == Q3_META_MISSING) return bad("metadata key '" + k + "' is missing");
        if (s == Q3_META_TYPE) return bad("metadata key '" + k + "' is not a float");
        if (!std::isfinite(v)) return bad("metadata key '" + k + "' is not finite");
        *out = (float)v;
        return 0;
    }
    // an integer array of lo_n .. cap entries, each 1 .. 4096; entries past its length are 0
    int ints(const char* k0, int lo_n, int cap, int32_t* n, int32_t* out) {
        const std::string k = key(k0);
        std::vector<int64_t> v;
        const int s = g.meta_int_array(k, &v);
        if (s == Q3_META_MISSING) return bad("metadata key '" + k + "' is missing");
        if (s == Q3_META_TYPE) return bad("metadata key '" + k + "' is not an integer array");
        if ((int64_t)v.size() < lo_n || (int64_t)v.size() > cap)
            return bad("metadata key '" + k + "' has " + std::to_string(v.size()) + " entries, " + (lo_n == cap ? std::to_string(cap) : std::to_string(lo_n) + " .. " + std::to_string(cap)) + " are needed");
        for (int i = 0; i < cap; ++i) out[i] = 0;
        for (size_t i = 0; i < v.size(); ++i) {
            if (v[i] < 1 || v[i] > 4096) return bad("metadata key '" + k + "' entry " + std::to_string(i) + " = " + std::to_string(v[i]) + " is out of range");
            out[i] = (int32_t)v[i];
        }
        if (n) *n = (int32_t)v.size();
        return 0;
    }
};

int cf_read_meta(const Q3CloneFiles& f, q3tts_clone_config* c, std::string& err) {
    CfMeta s{f.spk, f.spk_path, kSpkArch, err};
    if (s.check_arch() || s.integer("mel_dim", 1, &c->mel_dim) || s.ints("channels", 5, 5, nullptr, c->se_channels) ||
        s.ints("kernel_sizes", 5, 5, nullptr, c->se_kernels) || s.ints("dilations", 5, 5, nullptr, c->se_dilations) ||
        s.integer("attention_channels", 1, &c->se_attn_channels) || s.integer("res2net_scale", 1, &c->se_res2net_scale) ||
        s.integer("se_channels", 1, &c->se_se_channels) || s.integer("embedding_length", 1, &c->se_dim)) return -1;
    CfMeta a{f.codec, f.codec_path, kCodecArch, err};
    if (a.check_arch() || a.integer("filters", 1, &c->ae_filters) || a.integer("kernel_size", 1, &c->ae_kernel) ||
        a.integer("residual_kernel_size", 1, &c->ae_res_kernel) || a.integer("last_kernel_size", 1, &c->ae_last_kernel) ||
        a.ints("ratios", 1, 4, &c->ae_n_ratios, c->ae_ratios) || a.integer("embedding_length", 1, &c->ae_hidden) ||
        a.integer("block_count", 0, &c->ae_n_layer) || a.integer("attention.head_count", 1, &c->ae_n_head) ||
        a.integer("attention.key_length", 1, &c->ae_head_dim) || a.integer("feed_forward_length", 1, &c->ae_d_ffn) ||
        a.integer("attention.sliding_window", 1, &c->ae_window) || a.real("rope.freq_base", &c->ae_rope_theta) ||
        a.real("attention.layer_norm_epsilon", &c->ae_ln_eps) || a.integer("down_stride", 1, &c->ae_down_stride) ||
        a.integer("vq_dim", 1, &c->ae_vq_dim) || a.integer("n_codebooks", 1, &c->ae_n_codebooks) || a.integer("codebook_size", 1, &c->ae_codebook_size)) return -1;
    // the generator's ids leave AC_DOWN - AC_TFM layers and 256 - AC_CODEBOOK tables their own numbers
    if (c->ae_n_layer > AC_DOWN - AC_TFM) return a.bad("metadata key '" + a.key("block_count") + "' = " + std::to_string(c->ae_n_layer) + " is out of range");
    if (c->ae_n_codebooks > 256 - AC_CODEBOOK) return a.bad("metadata key '" + a.key("n_codebooks") + "' = " + std::to_string(c->ae_n_codebooks) + " is out of range");
    if (c->ae_filters > (1 << 16)) return a.bad("metadata key '" + a.key("filters") + "' = " + std::to_string(c->ae_filters) + " is out of range");
    return 0;
}

// one id as the device's array (see q3_clone_file_array)
int cf_array(const Q3CloneFiles& f, const CfSpec& s, const Q3GgufTensor* const* t, std::vector<float>& tmp, std::vector<float>& out, std::string& err) {
    auto fail = [&]() { err = cf_path(f, s) + ": " + err; return -1; };
    if (s.kind == CF_VEC || s.kind == CF_BOOK) {
        out.resize(t[0]->nelem);
        return q3_gguf_to_f32(*t[0], out.data(), err) ? fail() : 0;
    }
    const size_t N = (size_t)s.shape[0], CI = (size_t)s.shape[1], K = s.kind == CF_CONV ? (size_t)s.shape[2] : 1, kp = (size_t)cf_round512((int64_t)(K * CI));
    out.assign(s.names.size() * N * kp, 0.0f);
    for (size_t part = 0; part < s.names.size(); ++part) {
        tmp.resize(t[part]->nelem);
        if (q3_gguf_to_f32(*t[part], tmp.data(), err)) return fail();
        float* o = out.data() + part * N * kp;
        for (size_t n = 0; n < N; ++n) for (size_t ci = 0; ci < CI; ++ci) for (size_t k = 0; k < K; ++k) {
            const uint32_t u = (uint32_t)f32_to_bf16_rne(tmp[(n * CI + ci) * K + k]) << 16;
            memcpy(&o[n * kp + k * CI + ci], &u, 4);
        }
    }
    return 0;
}

}  // namespace

int q3_clone_files_open(const std::string& wdir, Q3CloneFiles& f, std::string& err) {
    f.spk_path = file_beside_model(wdir, Q3_SPK_FILE_NAME); f.codec_path = file_beside_model(wdir, Q3_CODEC_FILE_NAME);
    if (f.spk_path.empty() || f.codec_path.empty()) {
        const std::string where = " in " + wdir + " or its parent directory";
        if (f.spk_path.empty() && f.codec_path.empty()) err = std::string(Q3_SPK_FILE_NAME) + " and " + Q3_CODEC_FILE_NAME + " not found" + where;
        else if (f.spk_path.empty()) err = std::string(Q3_SPK_FILE_NAME) + " not found" + where + " (its partner is " + f.codec_path + "; the clone encoders need both files)";
        else err = std::string(Q3_CODEC_FILE_NAME) + " not found" + where + " (its partner is " + f.spk_path + "; the clone encoders need both files)";
        return 1;
    }
    if (f.spk.open(f.spk_path, err) || f.codec.open(f.codec_path, err)) return 2;
    return 0;
}

int q3_clone_file_config(const Q3CloneFiles& f, q3tts_clone_config* cc, std::string& err) {
    q3tts_clone_config c = *cc;  // (*cc is written only on success; ae_layer_scale is no file's to state)
    if (cf_read_meta(f, &c, err)) return -1;
    auto count = [&](bool codec, const char* key, int64_t want, const std::string& prefix, const std::string& suffix) {
        const int64_t have = vf_count(codec ? f.codec : f.spk, prefix, suffix);
        if (have == want) return 0;
        err = (codec ? f.codec_path : f.spk_path) + ": metadata key '" + (codec ? kCodecArch : kSpkArch) + "." + key + "' implies " + std::to_string(want) + " tensors '" + prefix + "N" + suffix + "...', the file has " + std::to_string(have);
        return -1;
    };
    for (int i = 1; i <= 3; ++i)
        if (count(false, "res2net_scale", c.se_res2net_scale - 1, "blocks." + std::to_string(i) + ".res2net_block.blocks.", ".conv.weight")) return -1;
    if (count(true, "ratios", c.ae_n_ratios, "encoder.layers.", ".block.1.conv.weight") || count(true, "block_count", c.ae_n_layer, "encoder_transformer.layers.", ".") ||
        count(true, "n_codebooks", c.ae_n_codebooks, "quantizer.codebook.", ".weight")) return -1;
    for (const auto& id : cf_ids(c)) {
        CfSpec s; const Q3GgufTensor* t[3];
        if (!cf_spec(c, id.first, id.second, &s)) { err = "no tensor for id (" + std::to_string(id.first) + ", " + std::to_string(id.second) + ")"; return -1; }
        if (cf_tensors(f, s, "the file's metadata implies", t, err)) return -1;
    }
    *cc = c;
    return 0;
}

int q3_clone_file_check(const Q3CloneFiles& f, const q3tts_clone_config& cc, std::string& err) {
    std::vector<float> buf;
    for (const auto& id : cf_ids(cc)) {
        CfSpec s; const Q3GgufTensor* t[3];
        if (!cf_spec(cc, id.first, id.second, &s)) { err = "no tensor for id (" + std::to_string(id.first) + ", " + std::to_string(id.second) + ")"; return -1; }
        if (cf_tensors(f, s, "the configuration needs", t, err)) return -1;
        for (size_t p = 0; p < s.names.size(); ++p) {
            buf.resize(t[p]->nelem);
            if (q3_gguf_to_f32(*t[p], buf.data(), err)) { err = cf_path(f, s) + ": " + err; return -1; }
            for (size_t i = 0; i < buf.size(); ++i)
                if (!std::isfinite(buf[i])) { err = cf_path(f, s) + ": tensor '" + s.names[p] + "' holds a value that is not finite (element " + std::to_string(i) + ")"; return -1; }
        }
    }
    return 0;
}

int q3_clone_file_array(const Q3CloneFiles& f, const q3tts_clone_config& cc, int comp, int which, std::vector<float>& out, std::string& err) {
    CfSpec s; const Q3GgufTensor* t[3];
    if (!cf_spec(cc, comp, which, &s)) { err = "the clone encoders' shape has no tensor of id (" + std::to_string(comp) + ", " + std::to_string(which) + ")"; return -1; }
    if (cf_tensors(f, s, "the configuration needs", t, err)) return -1;
    std::vector<float> tmp;
    return cf_array(f, s, t, tmp, out, err);
}

static void cf_copy_err(const std::string& msg, char* err, int32_t err_cap) {
    if (err && err_cap > 0) { const size_t n = msg.size() < (size_t)err_cap - 1 ? msg.size() : (size_t)err_cap - 1; memcpy(err, msg.data(), n); err[n] = '\0'; }
}

extern "C" int q3tts_clone_files_find(const char* weights_dir, char* speaker_path, char* codec_path, int32_t cap) {
    if (!weights_dir || !speaker_path || !codec_path || cap < 1) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    const std::string found[2] = {file_beside_model(weights_dir, Q3_SPK_FILE_NAME), file_beside_model(weights_dir, Q3_CODEC_FILE_NAME)};
    char* const out[2] = {speaker_path, codec_path};
    for (int i = 0; i < 2; ++i)
        if (found[i].size() + 1 > (size_t)cap) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "path buffer too small: " + std::to_string(found[i].size() + 1) + " bytes are needed");
    for (int i = 0; i < 2; ++i) memcpy(out[i], found[i].c_str(), found[i].size() + 1);
    return (found[0].empty() ? 0 : 1) + (found[1].empty() ? 0 : 1);
}

extern "C" int q3tts_clone_config_from_dir(const char* weights_dir, q3tts_clone_config* cfg, char* err, int32_t err_cap) {
    std::string msg;
    auto done = [&](int rc) { cf_copy_err(msg, err, err_cap); return rc; };
    if (!weights_dir || !cfg) { msg = "null argument"; return done(Q3TTS_ERR_INVALID); }
    Q3CloneFiles f;
    if (q3_clone_files_open(weights_dir, f, msg)) return done(Q3TTS_ERR_IO);
    return done(q3_clone_file_config(f, cfg, msg) ? Q3TTS_ERR_INVALID : Q3TTS_OK);
}

extern "C" int q3tts_k_clone_file_tensor(const char* weights_dir, const q3tts_clone_config* cfg, int32_t comp, int32_t which, float* out, int64_t cap, int64_t* n) {
    if (!weights_dir || !cfg || !n) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    std::string err;
    Q3CloneFiles f;
    if (q3_clone_files_open(weights_dir, f, err)) return q3_set_err(nullptr, Q3TTS_ERR_IO, err);
    std::vector<float> a;
    if (q3_clone_file_array(f, *cfg, comp, which, a, err)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, err);
    *n = (int64_t)a.size();
    if (out) {
        if (cap < *n) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "output buffer too small");
        memcpy(out, a.data(), a.size() * 4);
    }
    return Q3TTS_OK;
}
