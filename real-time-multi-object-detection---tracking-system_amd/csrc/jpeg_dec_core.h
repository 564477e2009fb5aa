// jpeg_dec_core.h -- the stream side of the baseline JPEG decoder: header parsing and validation, derived Huffman tables and the
// entropy decoder of ONE restart interval.  __host__ __device__, no HIP call in it: jpeg_dec.hip compiles it into the entropy kernel
// (jd_decode_interval) and into the host-side parser (jd_parse, also behind rtmodt_jpeg_probe); tests/native/jpeg_dec_check.cpp
// compiles the same file for the host alone and runs it under the sanitizers.  tests/jpeg_dec_ref.py restates every rule below.
//
// Accepted: SOF0, 8-bit samples, 8-bit quantisation tables, 1 or 3 components, one interleaved scan over all components (Ss 0, Se 63,
// Ah = Al = 0), luminance sampling 1x1 / 2x1 / 2x2 with 1x1 chrominance, at most four distinct Huffman tables in the scan, any DRI,
// sides 1..8192.  One component is decoded as 1x1 whatever its factors say.  A scan that names a Huffman table (class, 0 or 1) that
// no DHT defined uses the Annex K table of that class and number, as libjpeg does (AVI MJPG files carry no DHT).
// Statuses: UNSUPPORTED (the message names what), CORRUPT (broken structure, a DHT that is no prefix code, undefined tables),
// TRUNCATED (the file ends inside the header, or an interval consumed bits behind its end).
//
// Scan: [end of the SOS header, end of file) without a closing FF D9.  An interval's bits are its bytes with FF 00 -> FF up to the first
// FF that is not followed by 00 (or its end); behind them the reader supplies zero bits and the interval is TRUNCATED if it consumed
// one.  A code that does not resolve in 16 bits, a DC category above 11, an AC category above 10 or an index above 63: CORRUPT, the
// interval stops.  No read leaves [p, end); no write leaves the blocks of the interval's own MCUs.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace rtmodt {

#define JD_HD __host__ __device__

enum { JD_OK = 0, JD_UNSUPPORTED = 1, JD_CORRUPT = 2, JD_TRUNCATED = 3, JD_SIZE_MISMATCH = 4 };
constexpr int JD_MAX_DIM = 8192;

// a derived table (T.81 F.2.2.3): codes of up to 8 bits through `look`, longer ones through the maxcode / valoff walk
struct JdHuff {
    int32_t maxcode[18];        // [l], l = 1..16: the largest code of length l, -1 if none
    int32_t valoff[18];         // [l]: index into vals of the first code of length l, minus that code
    uint16_t look[256];         // next 8 bits -> length << 8 | symbol; 0: the code is longer
    uint8_t vals[256];
};

struct JdHeader {
    int32_t status;
    int32_t h, w, ncomp, hs, vs, ri;            // hs x vs: the luminance sampling (1 x 1 for one component)
    int32_t mcus_x, mcus_y, intervals;          // intervals = ceil(MCUs / ri), 1 without DRI
    uint32_t scan_off, scan_end;                // the entropy-coded bytes, relative to the file
    uint8_t comp_id[4], tq[4], slot_dc[4], slot_ac[4];
    uint8_t qt[4][64];                          // natural order
    JdHuff huff[4];                             // the (at most four) tables the scan uses; slot_dc / slot_ac index them
};

// where the blocks of a frame lie: component c owns bcols[c] x (mcus_y * v) blocks of 64 int16 from block comp_blk[c] on
struct JdLayout {
    uint32_t comp_blk[4], bcols[4];
};

JD_HD inline void jd_zigzag_fill(uint8_t *zz) {          // zz[k] = natural index of the k-th coefficient in zigzag order
    int r = 0, c = 0;
    for (int k = 0; k < 64; ++k) {
        zz[k] = (uint8_t)(r * 8 + c);
        if ((r + c) & 1) {                                 // moving down-left
            if (r == 7) ++c;
            else if (c == 0) ++r;
            else { ++r; --c; }
        } else {                                           // moving up-right
            if (c == 7) ++r;
            else if (r == 0) ++c;
            else { --r; ++c; }
        }
    }
}

// bits[16] counts per length, vals: the symbols.  false: no prefix code (libjpeg's test: a code of length l stays below 2^l)
JD_HD inline bool jd_derive(const uint8_t *bits, const uint8_t *vals, int nvals, JdHuff &t) {
    for (int i = 0; i < 256; ++i) {
        t.look[i] = 0;
        t.vals[i] = i < nvals ? vals[i] : 0;
    }
    int code = 0, k = 0;
    t.maxcode[0] = -1; t.valoff[0] = 0;
    t.maxcode[17] = 0x7fffffff; t.valoff[17] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = bits[l - 1];
        if (code + n > (1 << l)) return false;
        t.valoff[l] = k - code;
        if (l <= 8)
            for (int i = 0; i < n; ++i)
                for (int f = 0; f < (1 << (8 - l)); ++f) t.look[((code + i) << (8 - l)) + f] = (uint16_t)(l << 8 | t.vals[k + i]);
        code += n;
        k += n;
        t.maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    return true;
}

JD_HD inline void jd_std_table(int cls, int id, uint8_t *bits, uint8_t *vals, int &nvals) {      // T.81 Annex K.3
    const uint8_t dc_bits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
    const uint8_t ac_bits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
    const uint8_t ac_head[2][42] = {
        {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
         0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18},
        {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
         0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25}};
    // the rest of the two AC lists is made of runs lo..hi
    const uint8_t ac_runs[2][16][2] = {
        {{0x19, 0x1a}, {0x25, 0x2a}, {0x34, 0x3a}, {0x43, 0x4a}, {0x53, 0x5a}, {0x63, 0x6a}, {0x73, 0x7a}, {0x83, 0x8a}, {0x92, 0x9a},
         {0xa2, 0xaa}, {0xb2, 0xba}, {0xc2, 0xca}, {0xd2, 0xda}, {0xe1, 0xea}, {0xf1, 0xfa}, {1, 0}},
        {{0xf1, 0xf1}, {0x17, 0x1a}, {0x26, 0x2a}, {0x35, 0x3a}, {0x43, 0x4a}, {0x53, 0x5a}, {0x63, 0x6a}, {0x73, 0x7a}, {0x82, 0x8a},
         {0x92, 0x9a}, {0xa2, 0xaa}, {0xb2, 0xba}, {0xc2, 0xca}, {0xd2, 0xda}, {0xe2, 0xea}, {0xf2, 0xfa}}};
    id &= 1;
    nvals = 0;
    if (cls == 0) {
        for (int i = 0; i < 16; ++i) bits[i] = dc_bits[id][i];
        for (int i = 0; i < 12; ++i) vals[nvals++] = (uint8_t)i;
        return;
    }
    for (int i = 0; i < 16; ++i) bits[i] = ac_bits[id][i];
    for (int i = 0; i < 42; ++i) vals[nvals++] = ac_head[id][i];
    for (int r = 0; r < 16; ++r)
        for (int v = ac_runs[id][r][0]; v <= ac_runs[id][r][1]; ++v) vals[nvals++] = (uint8_t)v;
}

#define JD_FAIL(st, text) do { hd.status = (st); if (msg) *msg = (text); return (st); } while (0)

// Parses d[0, n) up to and including SOS.  Returns the status (also hd.status); *msg (optional) names the reason.  Every read is
// bounds-checked against n.  On a status other than JD_OK the rest of hd is unspecified.
JD_HD inline int jd_parse(const uint8_t *d, size_t n, JdHeader &hd, const char **msg) {
    struct Raw { uint8_t defined, bits[16], vals[256]; int nvals; };
    Raw raw[2][4];
    bool qt_defined[4] = {false, false, false, false}, have_sof = false;
    uint8_t zz[64], td[4] = {0, 0, 0, 0}, ta[4] = {0, 0, 0, 0};
    int adobe_transform = -1;
    jd_zigzag_fill(zz);
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 4; ++b) raw[a][b].defined = 0;
    hd.status = JD_OK; hd.ri = 0; hd.ncomp = 0; hd.h = hd.w = 0; hd.hs = hd.vs = 1;
    if (msg) *msg = "";
    if (n < 2) JD_FAIL(JD_TRUNCATED, "no SOI");
    if (d[0] != 0xFF || d[1] != 0xD8) JD_FAIL(JD_CORRUPT, "no SOI");
    size_t i = 2;
    for (;;) {
        if (i >= n) JD_FAIL(JD_TRUNCATED, "the file ends before SOS");
        if (d[i] != 0xFF) JD_FAIL(JD_CORRUPT, "no marker where one must be");
        while (i < n && d[i] == 0xFF) ++i;
        if (i >= n) JD_FAIL(JD_TRUNCATED, "the file ends before SOS");
        const int m = d[i++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) JD_FAIL(JD_CORRUPT, "a stand-alone marker in the header");
        if (i + 2 > n) JD_FAIL(JD_TRUNCATED, "the file ends inside a segment");
        const size_t L = (size_t)d[i] << 8 | d[i + 1];
        if (L < 2) JD_FAIL(JD_CORRUPT, "segment length below 2");
        if (i + L > n) JD_FAIL(JD_TRUNCATED, "the file ends inside a segment");
        const uint8_t *p = d + i + 2;
        const size_t pl = L - 2;
        i += L;
        if (m == 0xC0) {
            if (have_sof) JD_FAIL(JD_CORRUPT, "two SOF segments");
            if (pl < 6) JD_FAIL(JD_CORRUPT, "short SOF");
            const int prec = p[0], nc = p[5];
            hd.h = p[1] << 8 | p[2];
            hd.w = p[3] << 8 | p[4];
            if (prec == 12) JD_FAIL(JD_UNSUPPORTED, "12-bit samples");
            if (prec != 8) JD_FAIL(JD_UNSUPPORTED, "sample precision other than 8 bits");
            if (nc == 4) JD_FAIL(JD_UNSUPPORTED, "4 components");
            if (nc != 1 && nc != 3) JD_FAIL(JD_UNSUPPORTED, "a component count other than 1 or 3");
            if (pl != (size_t)(6 + 3 * nc)) JD_FAIL(JD_CORRUPT, "SOF length");
            if (hd.h == 0 || hd.w == 0) JD_FAIL(JD_CORRUPT, "empty frame");
            if (hd.h > JD_MAX_DIM || hd.w > JD_MAX_DIM) JD_FAIL(JD_UNSUPPORTED, "a frame side above 8192");
            int hsv[4][2];
            for (int c = 0; c < nc; ++c) {
                hd.comp_id[c] = p[6 + 3 * c];
                hsv[c][0] = p[7 + 3 * c] >> 4;
                hsv[c][1] = p[7 + 3 * c] & 15;
                hd.tq[c] = p[8 + 3 * c];
                if (hsv[c][0] < 1 || hsv[c][0] > 4 || hsv[c][1] < 1 || hsv[c][1] > 4) JD_FAIL(JD_CORRUPT, "sampling factor outside 1..4");
                if (hd.tq[c] > 3) JD_FAIL(JD_CORRUPT, "quantisation table number");
            }
            if (nc == 1) {
                hd.hs = hd.vs = 1;
            } else {
                hd.hs = hsv[0][0]; hd.vs = hsv[0][1];
                const bool luma_ok = (hd.hs == 1 && hd.vs == 1) || (hd.hs == 2 && hd.vs == 1) || (hd.hs == 2 && hd.vs == 2);
                if (!luma_ok || hsv[1][0] != 1 || hsv[1][1] != 1 || hsv[2][0] != 1 || hsv[2][1] != 1)
                    JD_FAIL(JD_UNSUPPORTED, "sampling other than 4:4:4, 4:2:2 or 4:2:0");
            }
            hd.ncomp = nc;
            have_sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4) {
            if (m == 0xC1) JD_FAIL(JD_UNSUPPORTED, "extended sequential stream");
            if (m == 0xC2) JD_FAIL(JD_UNSUPPORTED, "progressive stream");
            if (m == 0xC3) JD_FAIL(JD_UNSUPPORTED, "lossless stream");
            if (m == 0xCC) JD_FAIL(JD_UNSUPPORTED, "arithmetic coding");
            if (m > 0xC8) JD_FAIL(JD_UNSUPPORTED, "arithmetic-coded stream");
            JD_FAIL(JD_UNSUPPORTED, "differential stream");
        } else if (m == 0xDB) {
            for (size_t k = 0; k < pl; k += 65) {
                const int pq = p[k] >> 4, tq = p[k] & 15;
                if (pq == 1) JD_FAIL(JD_UNSUPPORTED, "16-bit quantisation table");
                if (pq > 1 || tq > 3 || k + 65 > pl) JD_FAIL(JD_CORRUPT, "DQT");
                for (int z = 0; z < 64; ++z) hd.qt[tq][zz[z]] = p[k + 1 + z];
                qt_defined[tq] = true;
            }
        } else if (m == 0xC4) {
            for (size_t k = 0; k < pl;) {
                const int tc = p[k] >> 4, th = p[k] & 15;
                if (tc > 1 || th > 3 || k + 17 > pl) JD_FAIL(JD_CORRUPT, "DHT");
                int cnt = 0;
                for (int b = 0; b < 16; ++b) cnt += p[k + 1 + b];
                if (cnt > 256 || k + 17 + (size_t)cnt > pl) JD_FAIL(JD_CORRUPT, "DHT");
                Raw &r = raw[tc][th];
                int code = 0;
                for (int l = 1; l <= 16; ++l) {
                    code += p[k + l];
                    if (code > (1 << l)) JD_FAIL(JD_CORRUPT, "DHT is no prefix code");
                    code <<= 1;
                }
                for (int b = 0; b < 16; ++b) r.bits[b] = p[k + 1 + b];
                for (int v = 0; v < cnt; ++v) r.vals[v] = p[k + 17 + v];
                r.nvals = cnt;
                r.defined = 1;
                k += 17 + (size_t)cnt;
            }
        } else if (m == 0xDD) {
            if (pl != 2) JD_FAIL(JD_CORRUPT, "DRI");
            hd.ri = p[0] << 8 | p[1];
        } else if (m == 0xEE) {
            if (pl >= 12 && p[0] == 'A' && p[1] == 'd' && p[2] == 'o' && p[3] == 'b' && p[4] == 'e') adobe_transform = p[11];
        } else if (m == 0xDA) {
            if (!have_sof) JD_FAIL(JD_CORRUPT, "SOS before SOF");
            if (pl < 1) JD_FAIL(JD_CORRUPT, "SOS");
            const int ns = p[0];
            if (ns < 1 || ns > 4 || pl != (size_t)(4 + 2 * ns)) JD_FAIL(JD_CORRUPT, "SOS");
            if (ns != hd.ncomp) JD_FAIL(JD_UNSUPPORTED, "multiple scans");
            for (int c = 0; c < ns; ++c) {
                if (p[1 + 2 * c] != hd.comp_id[c]) JD_FAIL(JD_UNSUPPORTED, "scan component order");
                td[c] = p[2 + 2 * c] >> 4;
                ta[c] = p[2 + 2 * c] & 15;
                if (td[c] > 3 || ta[c] > 3) JD_FAIL(JD_CORRUPT, "Huffman table number");
            }
            if (p[1 + 2 * ns] != 0 || p[2 + 2 * ns] != 63 || p[3 + 2 * ns] != 0)
                JD_FAIL(JD_UNSUPPORTED, "spectral selection / successive approximation");
            if (ns == 3 && adobe_transform == 0) JD_FAIL(JD_UNSUPPORTED, "Adobe transform 0 (RGB)");
            break;
        }
        // every other segment (APPn, COM, ...) is skipped
    }
    // the tables of the scan -> at most four slots
    int nslots = 0, slot_of[2][4];
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 4; ++b) slot_of[a][b] = -1;
    for (int c = 0; c < hd.ncomp; ++c) {
        if (!qt_defined[hd.tq[c]]) JD_FAIL(JD_CORRUPT, "undefined quantisation table");
        for (int cls = 0; cls < 2; ++cls) {
            const int id = cls ? ta[c] : td[c];
            if (slot_of[cls][id] < 0) {
                Raw &r = raw[cls][id];
                if (!r.defined) {
                    if (id > 1) JD_FAIL(JD_CORRUPT, "undefined Huffman table");
                    jd_std_table(cls, id, r.bits, r.vals, r.nvals);
                    r.defined = 1;
                }
                if (nslots == 4) JD_FAIL(JD_UNSUPPORTED, "more than four Huffman tables in one scan");
                if (!jd_derive(r.bits, r.vals, r.nvals, hd.huff[nslots])) JD_FAIL(JD_CORRUPT, "DHT is no prefix code");
                slot_of[cls][id] = nslots++;
            }
            (cls ? hd.slot_ac : hd.slot_dc)[c] = (uint8_t)slot_of[cls][id];
        }
    }
    hd.mcus_x = (hd.w + 8 * hd.hs - 1) / (8 * hd.hs);
    hd.mcus_y = (hd.h + 8 * hd.vs - 1) / (8 * hd.vs);
    const long long mcus = (long long)hd.mcus_x * hd.mcus_y;
    hd.intervals = hd.ri ? (int)((mcus + hd.ri - 1) / hd.ri) : 1;
    hd.scan_off = (uint32_t)i;
    hd.scan_end = (uint32_t)((n - 2 >= i && d[n - 2] == 0xFF && d[n - 1] == 0xD9) ? n - 2 : n);
    return JD_OK;
}
#undef JD_FAIL

// blocks of component c per MCU, and the layout of a frame's block array
JD_HD inline int jd_comp_h(const JdHeader &hd, int c) { return c == 0 ? hd.hs : 1; }
JD_HD inline int jd_comp_v(const JdHeader &hd, int c) { return c == 0 ? hd.vs : 1; }
JD_HD inline uint32_t jd_layout(const JdHeader &hd, JdLayout &lay) {       // returns the frame's blocks
    uint32_t at = 0;
    for (int c = 0; c < 4; ++c) {
        lay.comp_blk[c] = at;
        lay.bcols[c] = c < hd.ncomp ? (uint32_t)(hd.mcus_x * jd_comp_h(hd, c)) : 0;
        if (c < hd.ncomp) at += lay.bcols[c] * (uint32_t)(hd.mcus_y * jd_comp_v(hd, c));
    }
    return at;
}

// MSB-first bit reader over [p, end) with FF 00 unstuffing; behind the data it supplies zero bits and counts them.  Bytes are fetched
// up to the next 8-byte boundary of the address, so eight at a time after the first fetch (one load instead of eight dependent ones;
// the chunk after the current one is fetched ahead), never one at or behind `end`.
struct JdBits {
    const uint8_t *p, *end;       // p: the first byte not yet fetched
    uint64_t acc = 0;             // the next bits, left-aligned
    uint64_t raw = 0, nxt = 0;    // fetched bytes, the next one in the low byte: the chunk in use and the one behind it
    int raw_n = 0, nxt_n = 0;
    int n = 0, pad = 0;           // valid bits in acc; how many of them (at the tail) are supplied zeros
    bool done = false;
    JD_HD JdBits(const uint8_t *b, const uint8_t *e) : p(b), end(e) {
        fetch();
        refill();
    }
    JD_HD inline void fetch() {                                  // nxt <- the bytes from p up to the next 8-byte boundary, or to `end`
        const size_t left = (size_t)(end - p);
        int nb = 8 - (int)((uintptr_t)p & 7u);
        if ((size_t)nb > left) nb = (int)left;
        nxt = 0;
        if (nb == 8) __builtin_memcpy(&nxt, p, 8);                 // (little-endian: the first byte is the low one)
        else
            for (int i = 0; i < nb; ++i) nxt |= (uint64_t)p[i] << (8 * i);
        nxt_n = nb;
        p += nb;
    }
    JD_HD inline void refill() {
        raw = nxt;
        raw_n = nxt_n;
        if (raw_n) fetch();
    }
    JD_HD inline void fill() {                                   // afterwards n >= 32: a code (<= 16 bits) and its value (<= 11)
        if (n > 32) return;
        if (!done) {
            if (raw_n == 0) refill();
            const uint32_t x = (uint32_t)raw;
            if (raw_n >= 4 && ((((x & 0x7F7F7F7Fu) + 0x01010101u) & x & 0x80808080u) == 0)) {     // four bytes, none of them FF: all at once
                acc |= (uint64_t)__builtin_bswap32(x) << (32 - n);
                n += 32;
                raw >>= 32;
                raw_n -= 4;
                return;
            }
        }
        while (n <= 56) {
            uint32_t b = 0;
            if (!done) {
                if (raw_n == 0) refill();
                if (raw_n == 0) {
                    done = true;
                } else {
                    b = (uint32_t)(raw & 0xFFu);
                    raw >>= 8;
                    --raw_n;
                    if (b == 0xFFu) {
                        if (raw_n == 0) refill();
                        if (raw_n && (raw & 0xFFu) == 0) {       // FF 00: a data byte FF
                            raw >>= 8;
                            --raw_n;
                        } else {                                 // a marker, or FF as the last byte: the data ends here
                            done = true;
                            b = 0;
                        }
                    }
                }
            }
            if (done && pad < (1 << 24)) pad += 8;
            acc |= (uint64_t)b << (56 - n);
            n += 8;
        }
    }
    JD_HD inline uint32_t peek16() { fill(); return (uint32_t)(acc >> 48); }
    JD_HD inline void skip(int l) { acc <<= l; n -= l; }
    JD_HD inline uint32_t take(int l) { const uint32_t v = (uint32_t)(acc >> (64 - l)); skip(l); return v; }   // 1 <= l <= 16, after peek16 + skip
    JD_HD inline bool overrun() const { return n < pad; }
};

// one symbol; -1: no code of up to 16 bits matches
JD_HD inline int jd_symbol(JdBits &br, const JdHuff &t) {
    const uint32_t v = br.peek16();
    const uint32_t e = t.look[v >> 8];
    if (e) {
        br.skip((int)(e >> 8));
        return (int)(e & 255u);
    }
    for (int l = 9; l <= 16; ++l) {
        const int code = (int)(v >> (16 - l));
        if (code <= t.maxcode[l]) {
            br.skip(l);
            return t.vals[(code + t.valoff[l]) & 255];
        }
    }
    return -1;
}

JD_HD inline int jd_extend(uint32_t v, int s) { return v >= (1u << (s - 1)) ? (int)v : (int)v - (1 << s) + 1; }

// MCUs [first, first + count) of one frame from the bytes [p, end); nonzero coefficients go, in natural order, into the (zeroed)
// blocks of `coef` (the frame's block array) -- from the callers with `writer` set: a wave whose lanes all decode the SAME interval
// (every value then lives in scalar registers) lets one lane store.  Returns the interval's status.
JD_HD inline int jd_decode_interval(const uint8_t *p, const uint8_t *end, const JdHeader &hd, const JdHuff *tabs, const uint8_t *zz,
                                    const JdLayout &lay, long long first, long long count, int16_t *coef, bool writer = true) {
    // what the loops need of the header, read once (the stores below could alias it for all the compiler knows)
    const int ncomp = hd.ncomp, hs = hd.hs, vs = hd.vs, mcus_x = hd.mcus_x, mcus_y = hd.mcus_y;
    const uint32_t sdc = (uint32_t)hd.slot_dc[0] | (uint32_t)hd.slot_dc[1] << 8 | (uint32_t)hd.slot_dc[2] << 16;
    const uint32_t sac = (uint32_t)hd.slot_ac[0] | (uint32_t)hd.slot_ac[1] << 8 | (uint32_t)hd.slot_ac[2] << 16;
    const size_t blk0 = lay.comp_blk[0], blk1 = lay.comp_blk[1], blk2 = lay.comp_blk[2];
    const size_t cols0 = lay.bcols[0], cols1 = lay.bcols[1], cols2 = lay.bcols[2];
    JdBits br(p, end);
    int pred[4] = {0, 0, 0, 0};
    int my = (int)(first / mcus_x), mx = (int)(first % mcus_x);
    for (long long m = 0; m < count && my < mcus_y; ++m) {
        for (int c = 0; c < ncomp && c < 3; ++c) {
            const int ch = c == 0 ? hs : 1, cv = c == 0 ? vs : 1;
            const JdHuff &dc = tabs[(sdc >> (8 * c)) & 3u], &ac = tabs[(sac >> (8 * c)) & 3u];
            const size_t cblk = c == 0 ? blk0 : c == 1 ? blk1 : blk2, ccols = c == 0 ? cols0 : c == 1 ? cols1 : cols2;
            int pr = c == 0 ? pred[0] : c == 1 ? pred[1] : pred[2];
            for (int v = 0; v < cv; ++v)
                for (int h = 0; h < ch; ++h) {
                    if (br.overrun()) return JD_TRUNCATED;               // only zero bits from here on
                    int16_t *blk = coef + (cblk + (size_t)(my * cv + v) * ccols + (size_t)(mx * ch + h)) * 64;
                    int s = jd_symbol(br, dc);
                    if (s < 0 || s > 11) return br.overrun() ? JD_TRUNCATED : JD_CORRUPT;
                    if (s) pr = (int16_t)(pr + jd_extend(br.take(s), s));
                    if (pr && writer) blk[0] = (int16_t)pr;
                    for (int k = 1; k < 64;) {
                        const int rs = jd_symbol(br, ac);
                        if (rs < 0) return br.overrun() ? JD_TRUNCATED : JD_CORRUPT;
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (s) {
                            k += r;
                            if (k > 63 || s > 10) return br.overrun() ? JD_TRUNCATED : JD_CORRUPT;
                            const int val = jd_extend(br.take(s), s);
                            if (writer) blk[zz[k]] = (int16_t)val;
                            ++k;
                        } else if (r == 15) {
                            k += 16;
                        } else {
                            break;
                        }
                    }
                }
            if (c == 0) pred[0] = pr;
            else if (c == 1) pred[1] = pr;
            else pred[2] = pr;
        }
        if (++mx == mcus_x) { mx = 0; ++my; }
    }
    return br.overrun() ? JD_TRUNCATED : JD_OK;
}

}  // namespace rtmodt
