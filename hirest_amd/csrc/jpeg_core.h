// Baseline-JPEG arithmetic core shared by the host decoder (hirest_jpeg_decode_host) and the gfx950 kernels of
// jpeg.hip.  Every step is the integer recipe of libjpeg(-turbo) as Pillow drives it (Image.open(f).convert("RGB"):
// JDCT_ISLOW, fancy upsampling on, no merged upsampler), so the two decoders and Pillow agree bit for bit:
//   bit reader        0xFF00 unstuffing, RSTn, zero bits past the end of the scan (jdhuff.c fill_bit_buffer)
//   Huffman decode    8-bit look-ahead + maxcode / valoffset (jpeg_make_d_derived_tbl, jpeg_huff_decode)
//   IDCT              jpeg_idct_islow: 13-bit constants, PASS1_BITS = 2, DESCALE rounding, saturating range limit
//   upsampling        h2v1 / h2v2 triangle filters with alternating biases (jdsample.c), box when width <= 2
//   colour            build_ycc_rgb_table: 16 fraction bits, ONE_HALF rounding, clamped to 0..255
// Every load of compressed data is clamped into [scan_begin, scan_end) before it is made: corrupt input raises a flag
// in the status word and never reads outside the file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPG_HD __host__ __device__ __forceinline__
#else
#define JPG_HD inline
#endif

// per-image status bits of the entropy decode (0 = clean); any bit sends the image to the host fallback
#define JPG_ST_BAD_CODE 1      // a code longer than 16 bits                                  (HIREST_JPEG_ST_*)
#define JPG_ST_COEF_OVERRUN 2  // a coefficient past index 63
#define JPG_ST_OUT_OF_DATA 4   // bits consumed past the end of the entropy-coded data
#define JPG_ST_BAD_RESTART 8   // an RSTn out of sequence, or a marker where RSTn belongs
#define JPG_ST_UNSUPPORTED 16  // the parser did not accept the file: never decoded

namespace jpg {

// A Huffman table in decoding form.  look[v] for the next 8 bits v: (length << 8) | symbol, length 0 = longer code.
struct DTable {
    uint16_t look[256];
    int32_t maxcode[18];   // [l] = largest code of length l, -1 if none; [17] sentinel
    int32_t valoff[18];    // symbol index of code c of length l = c + valoff[l]
    uint8_t vals[256];
};

// 'natural order' (row-major index) of zigzag index k (jutils.c jpeg_natural_order); each side keeps its own copy
#define JPG_NATURAL_ORDER {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, \
                           7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, \
                           39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// Builds `t` from the DHT counts / values.  Validation (over-subscribed code space, DC symbols > 15) is done by the
// parser before a table ever reaches here.
JPG_HD void build_dtable(const uint8_t* bits, const uint8_t* vals, DTable* t) {
    int code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = bits[l - 1];
        if (n) {
            t->valoff[l] = p - code;
            code += n;
            p += n;
            t->maxcode[l] = code - 1;
        } else {
            t->valoff[l] = 0;
            t->maxcode[l] = -1;
        }
        code <<= 1;
    }
    t->maxcode[0] = -1;
    t->valoff[0] = 0;
    t->maxcode[17] = 0x7fffffff;
    t->valoff[17] = 0;
    for (int i = 0; i < 256; ++i) t->vals[i] = vals[i];
}

// look-ahead entry for the 8-bit window v (the first length l <= 8 with v >> (8 - l) <= maxcode[l], as the slow
// decode would find it)
JPG_HD uint16_t look_entry(const DTable* t, int v) {
    for (int l = 1; l <= 8; ++l) {
        const int c = v >> (8 - l);
        if (c <= t->maxcode[l]) return (uint16_t)((l << 8) | t->vals[(c + t->valoff[l]) & 255]);
    }
    return 0;
}

// MSB-first bit reader over the entropy-coded bytes [pos, end) of one file.
struct BitReader {
    const uint8_t* data;
    int64_t pos, begin, end;
    uint64_t buf;     // the low `nbits` bits are the next bits, most significant first
    int nbits;
    int fake;         // zero bits appended after a marker / the end (libjpeg's insufficient-data padding)
    int marker;       // a marker (or the end of the data) stopped the reader
    int status;

#if defined(__HIP_DEVICE_COMPILE__)
    // device: bytes come out of an aligned 8-byte window (one load per 8 bytes of the stream instead of one per byte);
    // the caller guarantees `data` is 8-byte aligned and the file's last 8-byte word is readable
    uint64_t win;
    int64_t wpos;
    JPG_HD uint8_t at(int64_t i) {
        const int64_t j = i < begin ? begin : (i >= end ? end - 1 : i);   // clamp first, then load
        const int64_t w = j & ~(int64_t)7;
        if (w != wpos) {
            wpos = w;
            win = *(const uint64_t*)(data + w);
        }
        return (uint8_t)(win >> (8 * (j - w)));
    }
#else
    JPG_HD uint8_t at(int64_t i) {
        const int64_t j = i < begin ? begin : (i >= end ? end - 1 : i);   // clamp first, then load
        return data[j];
    }
#endif
    JPG_HD void init(const uint8_t* d, int64_t b, int64_t e) {
        data = d; pos = begin = b; end = e; buf = 0; nbits = 0; fake = 0; marker = 0; status = 0;
#if defined(__HIP_DEVICE_COMPILE__)
        wpos = -1;
        win = 0;
#endif
    }
    JPG_HD void fill() {
        while (nbits <= 56) {
            uint32_t byte = 0;
            if (marker || pos >= end) {
                marker = 1;
                fake += 8;
            } else {
                byte = at(pos);
                if (byte == 0xFF) {
                    int64_t q = pos + 1;
                    while (q < end && at(q) == 0xFF) ++q;          // fill bytes
                    const uint32_t nx = q < end ? at(q) : 0xD9;
                    if (nx == 0) {
                        pos = q + 1;
                    } else {                                       // a marker: stop in front of it
                        pos = q - 1;
                        marker = 1;
                        byte = 0;
                        fake += 8;
                    }
                } else {
                    ++pos;
                }
            }
            buf = (buf << 8) | byte;
            nbits += 8;
        }
    }
    JPG_HD uint32_t peek(int n) {
        if (nbits < n) fill();
        return (uint32_t)(buf >> (nbits - n)) & ((1u << n) - 1);
    }
    JPG_HD void skip(int n) {
        nbits -= n;
        if (nbits < fake) status |= JPG_ST_OUT_OF_DATA;
    }
    JPG_HD uint32_t get(int n) {
        if (n == 0) return 0;
        const uint32_t v = peek(n);
        skip(n);
        return v;
    }
    JPG_HD int decode(const DTable* t) {
        const uint32_t v = peek(16);
        const uint16_t e = t->look[v >> 8];
        if (e >> 8) {
            skip(e >> 8);
            return e & 255;
        }
        int l = 9;
        int code = (int)(v >> 7);
        while (code > t->maxcode[l]) {
            if (l == 16) {
                status |= JPG_ST_BAD_CODE;
                skip(16);
                return 0;
            }
            ++l;
            code = (int)(v >> (16 - l));
        }
        skip(l);
        return t->vals[(code + t->valoff[l]) & 255];
    }
    // ---- chunked decode: a position in the scan that a second reader can enter at ----
    // The position of the next bit as 8 * (offset of the raw byte that holds it) + (bits of that byte already taken); a
    // stuffed 0xFF counts at its 0xFF (the last one of a run of fill bytes).  8 * end once only padding is left.  The reader
    // only knows `pos`, the next byte to load, so the bytes still buffered are walked back over: cheap, and only asked for
    // near the end of a chunk.
    JPG_HD int64_t bit_position() {
        const int real = nbits - fake;                  // fake bits are the newest in the buffer
        if (marker && real <= 0) return end * 8;
        int64_t p = pos;
        for (int m = (real + 7) >> 3; m > 0; --m) {
            while (p - 1 > begin && at(p - 1) == 0xFF) --p;          // fill bytes: part of no data byte
            p -= (p - 2 >= begin && at(p - 1) == 0 && at(p - 2) == 0xFF) ? 2 : 1;
        }
        return p * 8 + ((8 - (real & 7)) & 7);
    }
    // Starts reading at `bitpos` (a value of bit_position(), or a guess) as if the bits before it had been consumed.
    JPG_HD void enter(const uint8_t* d, int64_t b, int64_t e, int64_t bitpos) {
        init(d, b, e);
        pos = bitpos >> 3;
        begin = pos < e ? pos : b;                      // nothing in front of the entry byte is looked at again
        const int off = (int)(bitpos & 7);
        if (off) {
            peek(off);
            nbits -= off;
        }
    }
    // RSTn: drop the buffered bits, find the marker, check its number
    JPG_HD void restart(int expect) {
        buf = 0; nbits = 0; fake = 0; marker = 0;
        while (pos + 1 < end && !(at(pos) == 0xFF && at(pos + 1) != 0 && at(pos + 1) != 0xFF)) ++pos;
        if (pos + 1 >= end || at(pos + 1) != 0xD0 + expect) {
            status |= JPG_ST_BAD_RESTART;
            return;
        }
        pos += 2;
    }
};

JPG_HD int extend(int r, int s) { return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r; }

// Decodes one 8x8 block.  `put(k, v)` receives each non-zero coefficient with its zigzag index k (DC first).
template <class Put>
JPG_HD void decode_block(BitReader& br, const DTable* dc, const DTable* ac, int& pred, Put&& put) {
    int s = br.decode(dc);
    int diff = s ? extend((int)br.get(s), s) : 0;
    pred += diff;
    put(0, pred);
    for (int k = 1; k < 64; ++k) {
        const int rs = br.decode(ac);
        const int r = rs >> 4;
        s = rs & 15;
        if (s) {
            k += r;
            const int v = extend((int)br.get(s), s);
            if (k > 63) {
                br.status |= JPG_ST_COEF_OVERRUN;
                return;
            }
            put(k, v);
        } else {
            if (r != 15) break;
            k += 15;
        }
    }
}

// ---- IDCT (jidctint.c jpeg_idct_islow) ----
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int32_t F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633,
                  F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

// one 1-D pass: in[0..7] -> out[0..7] before the descale (the caller shifts)
JPG_HD void idct_1d(int32_t i0, int32_t i1, int32_t i2, int32_t i3, int32_t i4, int32_t i5, int32_t i6, int32_t i7,
                    int32_t* o) {
    int32_t z1 = (i2 + i6) * F_0_541;
    const int32_t t2 = z1 - i6 * F_1_847;
    const int32_t t3 = z1 + i2 * F_0_765;
    const int32_t t0 = (int32_t)((uint32_t)(i0 + i4) << CONST_BITS);
    const int32_t t1 = (int32_t)((uint32_t)(i0 - i4) << CONST_BITS);
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int32_t a0 = i7, a1 = i5, a2 = i3, a3 = i1;
    z1 = a0 + a3;
    int32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int32_t z5 = (z3 + z4) * F_1_175;
    a0 *= F_0_298; a1 *= F_2_053; a2 *= F_3_072; a3 *= F_1_501;
    z1 *= -F_0_899; z2 *= -F_2_562; z3 *= -F_1_961; z4 *= -F_0_390;
    z3 += z5; z4 += z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    o[0] = t10 + a3; o[7] = t10 - a3;
    o[1] = t11 + a2; o[6] = t11 - a2;
    o[2] = t12 + a1; o[5] = t12 - a1;
    o[3] = t13 + a0; o[4] = t13 - a0;
}

JPG_HD int32_t descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

// column pass: 8 dequantised coefficients of one column -> 8 workspace values
JPG_HD void idct_col(const int32_t* c, int32_t* ws) {
    int32_t o[8];
    idct_1d(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], o);
#pragma unroll
    for (int i = 0; i < 8; ++i) ws[i] = descale(o[i], CONST_BITS - PASS1_BITS);
}

JPG_HD uint8_t range_limit(int32_t v) {   // v centred on 0
    v += 128;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// row pass: 8 workspace values of one row -> 8 samples
JPG_HD void idct_row(const int32_t* w, uint8_t* out) {
    int32_t o[8];
    idct_1d(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], o);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = range_limit(descale(o[i], CONST_BITS + PASS1_BITS + 3));
}

// ---- upsampling + colour (jdsample.c, jdcolor.c) ----
// `P(r, c)` reads the chroma plane; cw, ch = downsampled width / height.  Returns the full-resolution chroma sample of
// output pixel (x, y) for luma sampling hs x vs (chroma 1x1).
template <class Plane>
JPG_HD int chroma_at(const Plane& P, int x, int y, int hs, int vs, int cw, int ch) {
    if (hs == 1 && vs == 1) return P(y, x);
    const int c = x >> 1;
    const int cn = (x & 1) ? (c + 1 < cw ? c + 1 : c) : (c > 0 ? c - 1 : 0);
    if (cw <= 2) return P(vs == 2 ? y >> 1 : y, c);     // libjpeg-turbo's box upsampler for narrow components
    if (vs == 1) {
        const int v = P(y, c) * 3, n = P(y, cn);
        return (x & 1) ? (v + n + 2) >> 2 : (v + n + 1) >> 2;
    }
    const int r = y >> 1;
    const int r2 = (y & 1) ? (r + 1 < ch ? r + 1 : r) : (r > 0 ? r - 1 : 0);
    const int t = 3 * P(r, c) + P(r2, c);
    const int n = 3 * P(r, cn) + P(r2, cn);
    return (x & 1) ? (3 * t + n + 7) >> 4 : (3 * t + n + 8) >> 4;
}

JPG_HD uint32_t ycc_rgb(int y, int cb, int cr) {   // packed r | g << 8 | b << 16
    cb -= 128;
    cr -= 128;
    const int r = y + ((91881 * cr + 32768) >> 16);
    const int g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    const int b = y + ((116130 * cb + 32768) >> 16);
    const uint32_t R = r < 0 ? 0 : (r > 255 ? 255 : r), G = g < 0 ? 0 : (g > 255 ? 255 : g), B = b < 0 ? 0 : (b > 255 ? 255 : b);
    return R | (G << 8) | (B << 16);
}

}  // namespace jpg
