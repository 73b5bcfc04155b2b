// q3_split.cpp — the long-document splitter (include/q3tts.h, "long documents"): UTF-8 text -> byte spans with a break
// kind each, for a host in any language. Pure host code: no engine, no GPU. The rules are the header's; tests/_long_ref.py restates them.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/q3tts.h"
#include "q3_unicode_tables.h"

namespace {

int fail(char* err, int32_t cap, int code, const std::string& m) {
    if (err && cap > 0) { snprintf(err, (size_t)cap, "%s", m.c_str()); }
    return code;
}

bool in_ranges(const Q3URange* r, int n, uint32_t cp) {
    int lo = 0, hi = n - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        if (cp < r[mid].lo) hi = mid - 1; else if (cp > r[mid].hi) lo = mid + 1; else return true;
    }
    return false;
}
inline bool speakable(uint32_t c) { return in_ranges(Q3U_LETTER, Q3U_LETTER_N, c) || in_ranges(Q3U_NUMBER, Q3U_NUMBER_N, c); }
inline bool is_ws(uint32_t c) { return c == 0x20 || c == '\t' || c == '\r' || c == '\n' || c == 0xA0 || c == 0x3000; }
inline bool is_ascii_term(uint32_t c) { return c == '.' || c == '!' || c == '?'; }
inline bool is_term(uint32_t c) { return is_ascii_term(c) || c == 0x2026 || c == 0x3002 || c == 0xFF01 || c == 0xFF1F; }
inline bool is_closer(uint32_t c) {
    return c == '"' || c == '\'' || c == ')' || c == ']' || c == '}' || c == 0x201D || c == 0x2019 || c == 0x300D || c == 0x300F || c == 0xFF09 ||
           c == 0x3011 || c == 0x300B;
}
inline bool is_ascii_letter(uint32_t c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }

// code points with their byte offsets (offs has one entry more: n); false with *bad = the offending sequence's first byte
bool decode(const unsigned char* s, int64_t n, std::vector<uint32_t>& cps, std::vector<int64_t>& offs, int64_t* bad) {
    int64_t i = 0;
    while (i < n) {
        const unsigned char c = s[i];
        uint32_t cp; int len;
        if (c < 0x80) { cp = c; len = 1; }
        else if ((c >> 5) == 6) { cp = c & 0x1F; len = 2; }
        else if ((c >> 4) == 14) { cp = c & 0x0F; len = 3; }
        else if ((c >> 3) == 30) { cp = c & 0x07; len = 4; }
        else { *bad = i; return false; }
        if (i + len > n) { *bad = i; return false; }
        for (int k = 1; k < len; ++k) { const unsigned char d = s[i + k]; if ((d >> 6) != 2) { *bad = i; return false; } cp = (cp << 6) | (d & 0x3F); }
        if ((len == 2 && cp < 0x80) || (len == 3 && cp < 0x800) || (len == 4 && cp < 0x10000) || cp > 0x10FFFF || (cp >= 0xD800 && cp < 0xE000)) { *bad = i; return false; }
        cps.push_back(cp); offs.push_back(i);
        i += len;
    }
    offs.push_back(n);
    return true;
}

struct Unit { int b, e, kind; };  // code-point range [b, e) and the kind of its end

// the lone '.' at code point i: the ASCII letters directly before it are one letter, or one of the listed abbreviations
bool abbreviation(const std::vector<uint32_t>& c, int i) {
    int a = i;
    while (a > 0 && is_ascii_letter(c[a - 1])) --a;
    const int len = i - a;
    if (len == 1) return true;
    if (len < 2 || len > 4) return false;
    char w[5] = {0};
    for (int k = 0; k < len; ++k) w[k] = (char)(c[a + k] | 0x20);
    static const char* const list[] = {"mr", "mrs", "ms", "dr", "prof", "sr", "jr", "st", "vs"};
    for (const char* x : list) if (!strcmp(w, x)) return true;
    return false;
}

}  // namespace

extern "C" int q3tts_text_split(const char* utf8, int64_t n_bytes, int32_t target_bytes, int32_t max_bytes, q3tts_text_span* spans, int32_t cap,
                                int32_t* n_spans, char* err, int32_t err_cap) {
    if (!n_spans || n_bytes < 0 || (n_bytes > 0 && !utf8) || cap < 0 || (cap > 0 && !spans)) return fail(err, err_cap, Q3TTS_ERR_INVALID, "text split: null argument or negative length");
    *n_spans = 0;
    const int target = target_bytes ? target_bytes : 120, maxb = max_bytes ? max_bytes : 240;
    if (target < 16 || target > maxb || maxb > 4096) return fail(err, err_cap, Q3TTS_ERR_INVALID, "text split: 16 <= target_bytes <= max_bytes <= 4096");
    if (n_bytes > 0x7fffffffll) return fail(err, err_cap, Q3TTS_ERR_INVALID, "text split: more than 2^31 bytes");
    std::vector<uint32_t> c; std::vector<int64_t> off;
    int64_t bad = 0;
    if (!decode((const unsigned char*)utf8, n_bytes, c, off, &bad)) return fail(err, err_cap, Q3TTS_ERR_INVALID, "text split: invalid UTF-8 at byte " + std::to_string(bad));
    const int n = (int)c.size();

    // 1. raw units: cut after every sentence end and at every paragraph break
    std::vector<Unit> raw;
    int ub = 0, i = 0;
    while (i < n) {
        if (is_ws(c[i])) {
            int j = i, nl = 0;
            while (j < n && is_ws(c[j])) { nl += c[j] == '\n'; ++j; }
            if (nl >= 2) { raw.push_back(Unit{ub, i, Q3TTS_BREAK_PARAGRAPH}); ub = j; }
            i = j;
        } else if (is_term(c[i])) {
            int j = i; bool ascii = true;
            while (j < n && is_term(c[j])) { ascii = ascii && is_ascii_term(c[j]); ++j; }
            int k = j;
            while (k < n && is_closer(c[k])) ++k;
            bool counts = !ascii || k == n || is_ws(c[k]);
            if (counts && j - i == 1 && c[i] == '.' && abbreviation(c, i)) counts = false;
            if (counts) { raw.push_back(Unit{ub, k, Q3TTS_BREAK_SENTENCE}); ub = k; }
            i = k;
        } else ++i;
    }
    raw.push_back(Unit{ub, n, Q3TTS_BREAK_END});

    // 2. trimmed, the unspeakable ones dropped (a paragraph break moves to the unit before), the over-long ones cut
    std::vector<Unit> units;
    for (Unit u : raw) {
        while (u.b < u.e && is_ws(c[u.b])) ++u.b;
        while (u.e > u.b && is_ws(c[u.e - 1])) --u.e;
        bool any = false;
        for (int k = u.b; k < u.e && !any; ++k) any = speakable(c[k]);
        if (!any) {
            if (u.kind == Q3TTS_BREAK_PARAGRAPH && !units.empty()) units.back().kind = Q3TTS_BREAK_PARAGRAPH;
            continue;
        }
        int b = u.b;
        while (off[u.e] - off[b] > maxb) {
            const int64_t lim_lo = off[b] + maxb / 4, lim_hi = off[b] + maxb;
            int cut = -1, next = -1, kind = Q3TTS_BREAK_HARD;
            for (int k = b; k < u.e && off[k + 1] <= lim_hi; ++k) {  // the last clause mark whose end lies in (lim_lo, lim_hi]
                const uint32_t x = c[k];
                const bool mark = x == 0xFF0C || x == 0x3001 || x == 0xFF1B || x == 0xFF1A || ((x == ',' || x == ';' || x == ':') && k + 1 < n && is_ws(c[k + 1]));
                if (mark && off[k + 1] > lim_lo) { cut = next = k + 1; kind = Q3TTS_BREAK_CLAUSE; }
            }
            if (cut < 0)
                for (int k = b; k < u.e && off[k] <= lim_hi; ++k)  // the last whitespace that starts in the range
                    if (is_ws(c[k]) && off[k] > lim_lo) cut = next = k;
            if (cut < 0) {  // the largest code-point boundary <= lim_hi
                int k = b;
                while (k < u.e && off[k + 1] <= lim_hi) ++k;
                cut = next = k;
            }
            int pe = cut;
            while (pe > b && is_ws(c[pe - 1])) --pe;
            units.push_back(Unit{b, pe, kind});
            while (next < u.e && is_ws(c[next])) ++next;
            b = next;
        }
        units.push_back(Unit{b, u.e, u.kind});
    }

    // 3. greedy packing, never across a paragraph end
    std::vector<Unit> out;
    for (const Unit& u : units) {
        if (!out.empty() && out.back().kind != Q3TTS_BREAK_PARAGRAPH && off[u.e] - off[out.back().b] <= target) { out.back().e = u.e; out.back().kind = u.kind; }
        else out.push_back(u);
    }
    if (!out.empty()) out.back().kind = Q3TTS_BREAK_END;
    *n_spans = (int32_t)out.size();
    if ((size_t)cap < out.size()) return fail(err, err_cap, Q3TTS_ERR_INVALID, "text split: spans holds fewer than *n_spans entries");
    for (size_t k = 0; k < out.size(); ++k) spans[k] = q3tts_text_span{off[out[k].b], off[out[k].e], out[k].kind};
    return Q3TTS_OK;
}
