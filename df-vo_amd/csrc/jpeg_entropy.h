// Host half of the JPEG decode (include/dfvo_hip.h, dfvo_jpeg_probe / dfvo_jpeg_entropy_decode): marker parsing and the
// bit-serial Huffman pass of a baseline sequential file, into memory the caller owns -- a dfvo_jpeg_info header and behind it
// the quantised coefficients as int16 in natural (de-zigzagged) order, one 64-coefficient block after another per component in
// raster order of the component's padded block grid.  Dequantisation, IDCT, upsampling and colour are the device's (jpeg.hip).
// Plain C++17: no HIP, no globals, no allocation, re-entrant; a stand-alone program includes it as it is
// (tests/host_harness/jpeg_entropy_check.cpp).  Every read of the input is bounds-checked against its length and every write
// against the capacity; a capacity that is too small is an error, never a truncation.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/dfvo_hip.h"

namespace dfvo {
namespace jpeg {

static_assert(sizeof(dfvo_jpeg_info) <= DFVO_JPEG_HEADER_BYTES, "the header is the first DFVO_JPEG_HEADER_BYTES of the buffer");

static const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

enum { FAST_BITS = 10 };

struct Huff {
    bool defined = false;
    uint16_t fast[1 << FAST_BITS];  // (length << 8) | symbol for codes of at most FAST_BITS bits, 0: longer or absent
    int16_t fast_ac[1 << FAST_BITS];  // AC: value * 256 + run * 16 + (code length + size) where code and magnitude bits fit in
                                    // FAST_BITS and the value in 8 bits, else 0
    int32_t maxcode[18];            // largest code of each length, -1 where the length has none
    int32_t valoff[17];             // index of the length's first symbol minus its first code
    uint8_t vals[256];
};

struct Parsed {
    dfvo_jpeg_info info;
    uint8_t qdefined[4];
    uint16_t qtab[4][64];  // natural order
    uint8_t comp_tq[3], comp_td[3], comp_ta[3], comp_id[3], comp_h[3], comp_v[3];
    int restart_interval;
    size_t scan_pos;  // first byte of the entropy-coded data
};

struct State {
    Parsed p;
    Huff dc[4], ac[4];
};

static inline int fail(const char** reason, const char* why) {
    if (reason) *reason = why;
    return DFVO_ERR_JPEG;
}

static inline uint32_t be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }

static inline int build_huff(Huff& h, const uint8_t* counts, const uint8_t* vals, int nvals, const char** reason) {
    memset(h.fast, 0, sizeof(h.fast));
    memcpy(h.vals, vals, (size_t)nvals);
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        const int cnt = counts[len - 1];
        h.valoff[len] = k - (int32_t)code;
        if (code + (uint32_t)cnt > (1u << len)) return fail(reason, "DHT: the code lengths overfill the code space");
        for (int i = 0; i < cnt; i++, k++, code++)
            if (len <= FAST_BITS) {
                const uint32_t first = code << (FAST_BITS - len);
                for (uint32_t j = 0; j < (1u << (FAST_BITS - len)); j++) h.fast[first + j] = (uint16_t)((len << 8) | h.vals[k]);
            }
        h.maxcode[len] = cnt ? (int32_t)code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    for (uint32_t i = 0; i < (1u << FAST_BITS); i++) {
        h.fast_ac[i] = 0;
        const int len = h.fast[i] >> 8, run = (h.fast[i] >> 4) & 15, mag = h.fast[i] & 15;
        if (h.fast[i] && mag && len + mag <= FAST_BITS) {
            const uint32_t bits = ((i << len) & ((1u << FAST_BITS) - 1u)) >> (FAST_BITS - mag);
            const int32_t v = bits < (1u << (mag - 1)) ? (int32_t)bits - (int32_t)((1u << mag) - 1u) : (int32_t)bits;
            if (v >= -128 && v <= 127) h.fast_ac[i] = (int16_t)(v * 256 + run * 16 + len + mag);
        }
    }
    h.defined = true;
    return DFVO_OK;
}

// the markers up to and including SOS; `st` (the Huffman tables) may be null for a header-only probe
static inline int parse_headers(const uint8_t* d, size_t n, Parsed& p, State* st, const char** reason) {
    memset(&p, 0, sizeof(p));
    if (!d || n < 2 || d[0] != 0xFF || d[1] != 0xD8) return fail(reason, "not a JPEG: the bytes do not start with SOI (FF D8)");
    size_t pos = 2;
    bool have_sof = false;
    for (;;) {
        if (pos + 2 > n) return fail(reason, "data ends early: no SOS marker");
        if (d[pos] != 0xFF) return fail(reason, "corrupt: a marker was expected");
        while (pos < n && d[pos] == 0xFF) pos++;  // fill bytes
        if (pos >= n) return fail(reason, "data ends early: no SOS marker");
        const int m = d[pos++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // stand-alone markers
        if (m == 0xD9) return fail(reason, "data ends early: EOI before any scan");
        if (m == 0x00) return fail(reason, "corrupt: a marker was expected");
        if (pos + 2 > n) return fail(reason, "data ends early: inside a marker segment");
        const size_t len = be16(d + pos);
        if (len < 2 || pos + len > n) return fail(reason, "data ends early: inside a marker segment");
        const uint8_t* s = d + pos + 2;
        const size_t sl = len - 2;
        pos += len;
        if (m == 0xC0 || m == 0xC1 || m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) ||
            (m >= 0xCD && m <= 0xCF)) {
            if (m == 0xC2) return fail(reason, "progressive JPEG (SOF2): only baseline sequential (SOF0) is decoded");
            if (m >= 0xC9) return fail(reason, "arithmetic coding (SOF9..15): only baseline Huffman (SOF0) is decoded");
            if (m != 0xC0) return fail(reason, "extended, lossless or differential JPEG (SOFn): only baseline sequential (SOF0) is decoded");
            if (have_sof) return fail(reason, "corrupt: a second SOF marker");
            if (sl < 6) return fail(reason, "corrupt: SOF0 too short");
            if (s[0] == 12) return fail(reason, "12-bit samples: only 8-bit samples are decoded");
            if (s[0] != 8) return fail(reason, "sample precision is not 8 bits");
            const int h = (int)be16(s + 1), w = (int)be16(s + 3), nc = s[5];
            if (nc == 4) return fail(reason, "four components (CMYK / YCCK): one (grey) or three (YCbCr) are decoded");
            if (nc != 1 && nc != 3) return fail(reason, "component count is not 1 (grey) or 3 (YCbCr)");
            if (h == 0 || w == 0) return fail(reason, "image size 0 (DNL-defined height is not decoded)");
            if (sl < (size_t)(6 + 3 * nc)) return fail(reason, "corrupt: SOF0 too short");
            for (int c = 0; c < nc; c++) {
                p.comp_id[c] = s[6 + 3 * c];
                p.comp_h[c] = (uint8_t)(s[7 + 3 * c] >> 4);
                p.comp_v[c] = (uint8_t)(s[7 + 3 * c] & 15);
                p.comp_tq[c] = s[8 + 3 * c];
                if (p.comp_tq[c] > 3) return fail(reason, "corrupt: quantisation table index above 3");
                if (p.comp_h[c] < 1 || p.comp_h[c] > 4 || p.comp_v[c] < 1 || p.comp_v[c] > 4)
                    return fail(reason, "corrupt: sampling factor outside 1 .. 4");
            }
            int H = 1, V = 1;
            if (nc == 3) {
                H = p.comp_h[0];
                V = p.comp_v[0];
                const bool ok = ((H == 1 && V == 1) || (H == 2 && V == 1) || (H == 2 && V == 2)) && p.comp_h[1] == 1 &&
                                p.comp_v[1] == 1 && p.comp_h[2] == 1 && p.comp_v[2] == 1;
                if (!ok) return fail(reason, "sampling: luma 1x1, 2x1 or 2x2 with chroma 1x1 (4:4:4, 4:2:2, 4:2:0) is decoded, nothing else");
            }
            // (a one-component scan is not interleaved: its blocks cover the image whatever its sampling factors say)
            p.info.width = w;
            p.info.height = h;
            p.info.components = nc;
            p.info.h_samp = H;
            p.info.v_samp = V;
            const int mx = (w + 8 * H - 1) / (8 * H), my = (h + 8 * V - 1) / (8 * V);
            uint64_t off = DFVO_JPEG_HEADER_BYTES;
            for (int c = 0; c < nc; c++) {
                const int ch = c == 0 ? H : 1, cv = c == 0 ? V : 1;
                p.info.blocks_w[c] = mx * ch;
                p.info.blocks_h[c] = my * cv;
                p.info.comp_w[c] = (w * ch + H - 1) / H;
                p.info.comp_h[c] = (h * cv + V - 1) / V;
                p.info.plane_offset[c] = off;
                off += (uint64_t)p.info.blocks_w[c] * (uint64_t)p.info.blocks_h[c] * 128u;
            }
            p.info.bytes = off;
            have_sof = true;
        } else if (m == 0xDB) {  // DQT
            size_t q = 0;
            while (q < sl) {
                const int pq = s[q] >> 4, tq = s[q] & 15;
                if (pq == 1) return fail(reason, "16-bit quantisation tables: only 8-bit tables are decoded");
                if (pq != 0 || tq > 3) return fail(reason, "corrupt: DQT precision or table index");
                if (q + 65 > sl) return fail(reason, "corrupt: DQT too short");
                for (int k = 0; k < 64; k++) p.qtab[tq][ZIGZAG[k]] = s[q + 1 + k];
                p.qdefined[tq] = 1;
                q += 65;
            }
        } else if (m == 0xC4) {  // DHT
            size_t q = 0;
            while (q < sl) {
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) return fail(reason, "corrupt: DHT class or table index");
                if (q + 17 > sl) return fail(reason, "corrupt: DHT too short");
                int nv = 0;
                for (int k = 0; k < 16; k++) nv += s[q + 1 + k];
                if (nv > 256 || q + 17 + (size_t)nv > sl) return fail(reason, "corrupt: DHT too short");
                if (st) {
                    const int rc = build_huff(tc ? st->ac[th] : st->dc[th], s + q + 1, s + q + 17, nv, reason);
                    if (rc != DFVO_OK) return rc;
                }
                q += 17 + (size_t)nv;
            }
        } else if (m == 0xCC) {
            return fail(reason, "arithmetic coding (DAC): only baseline Huffman is decoded");
        } else if (m == 0xDD) {  // DRI
            if (sl < 2) return fail(reason, "corrupt: DRI too short");
            p.restart_interval = (int)be16(s);
        } else if (m == 0xDA) {  // SOS
            if (!have_sof) return fail(reason, "corrupt: SOS before SOF0");
            const int nc = p.info.components;
            if (sl < 1) return fail(reason, "corrupt: SOS too short");
            if (s[0] != nc) return fail(reason, "more than one scan: the one scan must interleave every component");
            if (sl < (size_t)(4 + 2 * nc)) return fail(reason, "corrupt: SOS too short");
            for (int c = 0; c < nc; c++) {
                if (s[1 + 2 * c] != p.comp_id[c]) return fail(reason, "corrupt: the scan's components are not the frame's, in order");
                p.comp_td[c] = (uint8_t)(s[2 + 2 * c] >> 4);
                p.comp_ta[c] = (uint8_t)(s[2 + 2 * c] & 15);
                if (p.comp_td[c] > 3 || p.comp_ta[c] > 3) return fail(reason, "corrupt: Huffman table index above 3");
                if (!p.qdefined[p.comp_tq[c]]) return fail(reason, "missing table: a component's quantisation table was never defined");
                if (st && (!st->dc[p.comp_td[c]].defined || !st->ac[p.comp_ta[c]].defined))
                    return fail(reason, "missing table: a component's Huffman table was never defined");
                memcpy(p.info.quant[c], p.qtab[p.comp_tq[c]], sizeof(p.info.quant[c]));
            }
            if (s[1 + 2 * nc] != 0 || s[2 + 2 * nc] != 63 || s[3 + 2 * nc] != 0)
                return fail(reason, "progressive scan parameters in SOS: only baseline sequential is decoded");
            p.scan_pos = pos;
            return DFVO_OK;
        }
        // APPn, COM and anything else with a length: skipped
    }
}

// the entropy-coded segment's bit reader: FF 00 is a data byte FF, any other FF xx ends the supply
struct Bits {
    const uint8_t* d;
    size_t n, pos;
    uint64_t acc = 0;  // the low `cnt` bits are valid
    int cnt = 0;
    Bits(const uint8_t* d_, size_t n_, size_t pos_) : d(d_), n(n_), pos(pos_) {}
    inline void fill() {
        if (cnt <= 16 && pos + 6 <= n) {  // six bytes at once where none of them is FF (nearly always)
            const uint64_t v = ((uint64_t)d[pos] << 40) | ((uint64_t)d[pos + 1] << 32) | ((uint64_t)d[pos + 2] << 24) |
                               ((uint64_t)d[pos + 3] << 16) | ((uint64_t)d[pos + 4] << 8) | (uint64_t)d[pos + 5];
            const uint64_t x = ~v | 0xFFFF000000000000ull;  // a byte of x is 0 where a byte of v is FF
            if (!((x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull)) {
                acc = (acc << 48) | v;
                cnt += 48;
                pos += 6;
                return;
            }
        }
        while (cnt <= 48) {
            if (pos >= n) return;
            const uint8_t b = d[pos];
            if (b == 0xFF) {
                if (pos + 1 >= n || d[pos + 1] != 0x00) return;  // a marker, or the end of the data
                pos += 2;
            } else {
                pos++;
            }
            acc = (acc << 8) | b;
            cnt += 8;
        }
    }
    // the next 16 bits, zeros where the data has ended (the caller checks what it consumed against cnt)
    inline uint32_t peek16() {
        if (cnt < 16) fill();
        return cnt >= 16 ? (uint32_t)(acc >> (cnt - 16)) & 0xFFFFu : (uint32_t)(acc << (16 - cnt)) & 0xFFFFu;
    }
    inline bool skip(int k) {
        if (k > cnt) return false;
        cnt -= k;
        return true;
    }
    inline bool get(int k, uint32_t* v) {  // 1 <= k <= 16
        if (cnt < k) {
            fill();
            if (cnt < k) return false;
        }
        cnt -= k;
        *v = (uint32_t)(acc >> cnt) & ((1u << k) - 1u);
        return true;
    }
};

enum { SYM_EARLY = -1, SYM_BAD = -2 };

static inline int decode_symbol(Bits& b, const Huff& h) {
    const uint32_t look = b.peek16();
    const uint16_t f = h.fast[look >> (16 - FAST_BITS)];
    if (f) return b.skip(f >> 8) ? (f & 255) : SYM_EARLY;
    for (int len = FAST_BITS + 1; len <= 16; len++) {
        const int32_t code = (int32_t)(look >> (16 - len));
        if (code <= h.maxcode[len]) {
            if (!b.skip(len)) return SYM_EARLY;
            const int32_t idx = code + h.valoff[len];
            return (idx >= 0 && idx < 256) ? h.vals[idx] : SYM_BAD;
        }
    }
    return b.cnt < 16 ? SYM_EARLY : SYM_BAD;
}

static inline int32_t extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int32_t)v - (int32_t)((1u << s) - 1u) : (int32_t)v; }

static inline int probe(const uint8_t* d, size_t n, dfvo_jpeg_info* info, const char** reason) {
    if (!info) return fail(reason, "null info");
    Parsed p;
    const int rc = parse_headers(d, n, p, nullptr, reason);
    if (rc == DFVO_OK) *info = p.info;
    return rc;
}

static inline int entropy_decode(const uint8_t* d, size_t n, void* dst, size_t capacity, dfvo_jpeg_info* info, const char** reason) {
    if (!dst || ((uintptr_t)dst & 7u)) return fail(reason, "destination is null or not 8-byte aligned");
    State st;
    Parsed& p = st.p;
    int rc = parse_headers(d, n, p, &st, reason);
    if (rc != DFVO_OK) return rc;
    if (p.info.bytes > (uint64_t)capacity) return fail(reason, "capacity too small: the header and coefficients need more bytes than the destination has");
    const int nc = p.info.components;
    uint8_t* out = (uint8_t*)dst;
    memset(out, 0, DFVO_JPEG_HEADER_BYTES);  // (every block is zeroed where it is decoded; on an error the rest stays as it was)
    memcpy(out, &p.info, sizeof(p.info));
    int16_t* plane[3] = {nullptr, nullptr, nullptr};
    for (int c = 0; c < nc; c++) plane[c] = (int16_t*)(out + p.info.plane_offset[c]);

    const int H = p.info.h_samp, V = p.info.v_samp;
    const int mx = p.info.blocks_w[0] / H, my = p.info.blocks_h[0] / V;
    Bits b(d, n, p.scan_pos);
    uint32_t pred[3] = {0, 0, 0};
    int until_restart = p.restart_interval, next_rst = 0;
    for (int my_i = 0; my_i < my; my_i++)
        for (int mx_i = 0; mx_i < mx; mx_i++) {
            if (p.restart_interval && until_restart == 0) {
                // whole bytes of padding are dropped with the bit buffer; the marker follows, after optional fill bytes
                if (b.cnt >= 8) return fail(reason, "bad restart marker: data where RSTn was expected");
                b.cnt = 0;
                size_t q = b.pos;
                if (q >= n) return fail(reason, "data ends early: inside the scan");
                if (d[q] != 0xFF) return fail(reason, "bad restart marker: data where RSTn was expected");
                while (q < n && d[q] == 0xFF) q++;
                if (q >= n) return fail(reason, "data ends early: inside the scan");
                if (d[q] != 0xD0 + next_rst) return fail(reason, "bad restart marker: not the RSTn that was due");
                b.pos = q + 1;
                next_rst = (next_rst + 1) & 7;
                until_restart = p.restart_interval;
                pred[0] = pred[1] = pred[2] = 0;
            }
            until_restart--;
            for (int c = 0; c < nc; c++) {
                const int ch = c == 0 ? H : 1, cv = c == 0 ? V : 1;
                const Huff& hd = st.dc[p.comp_td[c]];
                const Huff& ha = st.ac[p.comp_ta[c]];
                for (int v = 0; v < cv; v++)
                    for (int h = 0; h < ch; h++) {
                        int16_t* blk = plane[c] + ((size_t)(my_i * cv + v) * (size_t)p.info.blocks_w[c] + (size_t)(mx_i * ch + h)) * 64;
                        memset(blk, 0, 128);
                        int s = decode_symbol(b, hd);
                        if (s < 0) return fail(reason, s == SYM_EARLY ? "data ends early: inside the scan" : "Huffman code that is not in its table");
                        if (s > 15) return fail(reason, "corrupt: DC category above 15");
                        if (s) {
                            uint32_t bits;
                            if (!b.get(s, &bits)) return fail(reason, "data ends early: inside the scan");
                            pred[c] += (uint32_t)extend(bits, s);
                        }
                        blk[0] = (int16_t)(uint16_t)pred[c];
                        for (int k = 1; k < 64; k++) {
                            const int fa = ha.fast_ac[b.peek16() >> (16 - FAST_BITS)];
                            if (fa) {  // code and magnitude bits in one look-up
                                if (!b.skip((int)((unsigned)fa & 15u))) return fail(reason, "data ends early: inside the scan");
                                k += (int)(((unsigned)fa >> 4) & 15u);
                                if (k > 63) return fail(reason, "coefficient index past 63");
                                blk[ZIGZAG[k]] = (int16_t)(fa / 256 - (fa % 256 < 0));
                                continue;
                            }
                            const int rs = decode_symbol(b, ha);
                            if (rs < 0) return fail(reason, rs == SYM_EARLY ? "data ends early: inside the scan" : "Huffman code that is not in its table");
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;  // EOB
                                k += 15;
                                continue;
                            }
                            k += r;
                            if (k > 63) return fail(reason, "coefficient index past 63");
                            uint32_t bits;
                            if (!b.get(s, &bits)) return fail(reason, "data ends early: inside the scan");
                            blk[ZIGZAG[k]] = (int16_t)extend(bits, s);
                        }
                    }
            }
        }
    // behind the scan: EOI, nothing else that starts a scan
    size_t q = b.pos;
    for (;;) {
        while (q < n && d[q] != 0xFF) q++;  // (padding bytes a careless encoder left)
        while (q < n && d[q] == 0xFF) q++;
        if (q >= n) return fail(reason, "data ends early: no EOI marker");
        const int m = d[q++];
        if (m == 0xD9) break;
        if (m == 0xDA) return fail(reason, "more than one scan: the one scan must interleave every component");
        if (m == 0x00 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (q + 2 > n) return fail(reason, "data ends early: no EOI marker");
        const size_t len = be16(d + q);
        if (len < 2 || q + len > n) return fail(reason, "data ends early: no EOI marker");
        q += len;
    }
    if (info) *info = p.info;
    return DFVO_OK;
}

}  // namespace jpeg
}  // namespace dfvo
