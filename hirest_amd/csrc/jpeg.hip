// Baseline-JPEG decode for gfx950, bit-exact with Pillow's Image.open(f).convert("RGB") (libjpeg-turbo, JDCT_ISLOW,
// fancy upsampling).  The frames the reference encodes are JPEG files on disk (extract_features.py:45-49,
// inference_video_retrieval.py:35-46, written by extract_frames.py's cv2.imwrite: baseline, 4:2:0, q95).
//
// Host:   hirest_jpeg_parse reads the markers of one file into a descriptor + its raw tables; anything outside the
//         supported subset (progressive, arithmetic, 12-bit, CMYK / RGB, multi-scan, odd sampling, truncated) is
//         flagged and left to the caller's fallback.  hirest_jpeg_decode_host runs the same core on the CPU.
// Device: three kernels on the caller's stream.
//   jpeg_entropy_kernel   one lane per image, 16 per workgroup: Huffman decode of the whole scan (tables in LDS) -> int16
//                         coefficient blocks in component-plane block order; per-image status word.  Bounds the decoder
//                         (99.8 % of its GPU time).
//   jpeg_entropy_chunked_kernel  (hirest_jpeg_decode_chunked) the same coefficients from one workgroup of up to 1024 lanes per
//                         image, one lane per chunk of the scan, synchronised by re-entering from the neighbour's exit; images
//                         with a restart interval go to jpeg_entropy_restart_kernel, the one-lane code.
//   jpeg_idct_kernel      32 blocks per workgroup, one thread per block column (pass 1) and row (pass 2) ->
//                         uint8 component planes (MCU-padded).
//   jpeg_color_kernel     16 output pixels per thread: fancy upsampling + YCbCr -> RGB, 16-byte stores into the
//                         [H, W, 3] frame.
// Workspace (hirest_jpeg_workspace_bytes): the coefficient blocks of the <= 16 images of one entropy workgroup interleaved
// (block b of lane l at group + 128 l + 2048 b: lanes in lockstep store into one 2 KB span, not 16 pages apart), then
// nblocks * 64 B of component planes per image.
#include "common.h"
#include "jpeg_core.h"
#include <string.h>
#include <vector>

namespace {

constexpr int ENT_LANES = 16;      // images per entropy workgroup: few lanes per wave, so a batch spreads over many CUs
constexpr int IDCT_BLOCKS = 32;    // 8x8 blocks per IDCT workgroup (256 threads)
constexpr int COLOR_THREADS = 256;
constexpr int MAX_DIM = 16384;
constexpr int64_t COEF_STRIDE = ENT_LANES * 64;   // int16 elements between consecutive blocks of one image (interleaved lanes)

__constant__ uint8_t kNatural[64] = JPG_NATURAL_ORDER;

struct Geo {
    int bw0, bh0;             // luma (or grey) blocks per row / column, MCU-padded
    int64_t nblocks, off1, off2;   // total blocks; first block of Cb, Cr
};

JPG_HD Geo geo_of(const hirest_jpeg_image& d) {
    Geo g;
    g.bw0 = d.mcux * d.hs;
    g.bh0 = d.mcuy * d.vs;
    g.off1 = (int64_t)g.bw0 * g.bh0;
    g.off2 = g.off1 + (int64_t)d.mcux * d.mcuy;
    g.nblocks = d.ncomp == 3 ? g.off2 + (int64_t)d.mcux * d.mcuy : g.off1;
    return g;
}

JPG_HD int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// The whole scan of one image.  `blk(i)` returns the zeroed int16[64] of block i (component-plane order), `done(i)` is
// called when it is complete; `nat` is the natural-order table.  Returns the status bits.
template <class Block, class Done>
JPG_HD int decode_scan(const hirest_jpeg_image& d, const uint8_t* file, const jpg::DTable* dt, const uint8_t* nat, Block&& blk,
                       Done&& done) {
    const Geo g = geo_of(d);
    jpg::BitReader br;
    br.init(file, d.scan_begin, d.scan_end);
    int p0 = 0, p1 = 0, p2 = 0;
    int rst_left = d.restart_interval, next_rst = 0;
    const int ny = d.hs * d.vs, per_mcu = ny + (d.ncomp == 3 ? 2 : 0);
    for (int my = 0; my < d.mcuy; ++my) {
        for (int mx = 0; mx < d.mcux; ++mx) {
            if (d.restart_interval) {
                if (rst_left == 0) {
                    br.restart(next_rst);
                    next_rst = (next_rst + 1) & 7;
                    rst_left = d.restart_interval;
                    p0 = p1 = p2 = 0;
                }
                --rst_left;
            }
            for (int b = 0; b < per_mcu; ++b) {
                const int c = b < ny ? 0 : b - ny + 1;
                int64_t bi;
                if (c == 0) bi = (int64_t)(my * d.vs + (b >> (d.hs - 1))) * g.bw0 + mx * d.hs + (b & (d.hs - 1));
                else bi = (c == 1 ? g.off1 : g.off2) + (int64_t)my * d.mcux + mx;
                int16_t* out = blk(bi);
                int pred = c == 0 ? p0 : (c == 1 ? p1 : p2);
                jpg::decode_block(br, dt + 2 * c, dt + 2 * c + 1, pred, [&](int k, int v) { out[nat[k]] = (int16_t)v; });
                done(bi);
                if (c == 0) p0 = pred; else if (c == 1) p1 = pred; else p2 = pred;
            }
            if (br.status) return br.status;
        }
    }
    return br.status;
}

// ---- chunked entropy decode (restart_interval == 0): many lanes per image ----
// The scan is cut into chunks of `cb` bytes, one lane each.  A lane owns the blocks whose first bit lies in its chunk and
// decodes each of them to its end.  Sync pass: lane 0 enters at scan_begin, every other lane guesses that a block (the first
// of an MCU) starts at its first bit; each records where it leaves (the first block start at or past its chunk's end), how
// many blocks it owns and the sums of their DC differences.  Then lane i + 1 re-enters from lane i's exit until no exit
// changes: lane 0 is exact, so after r rounds lanes 0 .. r - 1 are, and the fixed point is the serial decode.  An exclusive
// scan of (blocks, DC sums) gives each lane its first block and predictors, and the write pass decodes the owned blocks again,
// this time with output.  Blocks past the image's last one (the padding bits can look like one) are nobody's.
constexpr int CHUNK_MAX_LANES = 1024;   // lanes of one image = threads of its workgroup
constexpr int CHUNK_MIN_BYTES = 256;    // chosen chunk size: not below this (a lane runs on into the next chunk to the end of
                                        // its last block, and a wrong guess costs a round)

// chunk size for a scan of `len` bytes: the caller's, else the smallest >= CHUNK_MIN_BYTES that fits max_lanes; a caller's
// size that needs more than max_lanes is raised to fit
JPG_HD int64_t chunk_size(int64_t len, int64_t want, int64_t max_lanes) {
    const int64_t fit = (len + max_lanes - 1) / max_lanes;
    const int64_t cb = want > 0 ? want : CHUNK_MIN_BYTES;
    return cb > fit ? cb : fit;
}

// a lane's entry or exit: bit position (jpg::BitReader::bit_position) * 8 + index of the block inside its MCU
JPG_HD int64_t chunk_state(int64_t bitpos, int b) { return bitpos * 8 + b; }

// the first guess of lane `lane`: its chunk's first byte, or the next one if that is the stuffed 0x00 of an 0xFF
JPG_HD int64_t chunk_guess(const hirest_jpeg_image& d, const uint8_t* file, int64_t cb, int64_t lane) {
    int64_t s = d.scan_begin + lane * cb;
    if (lane > 0 && file[s] == 0 && file[s - 1] == 0xFF) ++s;
    return chunk_state(s * 8, 0);
}

struct ChunkOut {
    int64_t exit;        // chunk_state where the lane stopped
    int32_t nown;        // blocks decoded
    int32_t dc[3];       // predictors after the last block (sync pass: from 0, i.e. the sums of the DC differences)
    int32_t status;
};

// One lane: enters at `entry`, decodes blocks while they start before bit `end_bits`.  WRITE: `first` is the scan-order
// index of its first block and o->dc its predictors; blocks go through blk / done as in decode_scan and the lane stops at
// the image's last block.  Without WRITE nothing is stored and anomalies are not reported.
template <bool WRITE, class Block, class Done>
JPG_HD void decode_chunk(const hirest_jpeg_image& d, const Geo& g, const uint8_t* file, const jpg::DTable* dt, const uint8_t* nat,
                         int64_t entry, int64_t end_bits, int64_t first, ChunkOut* o, Block&& blk, Done&& done) {
    const int ny = d.hs * d.vs, per_mcu = ny + (d.ncomp == 3 ? 2 : 0);
    jpg::BitReader br;
    br.enter(file, d.scan_begin, d.scan_end, entry >> 3);
    int b = (int)(entry & 7), n = 0;
    int mx = 0, my = 0;
    if (WRITE) {
        const int64_t mcu = first / per_mcu;
        b = (int)(first - mcu * per_mcu);      // equal to the entry's once the sync pass has converged; this one bounds the stores
        my = (int)(mcu / d.mcux);
        mx = (int)(mcu - (int64_t)my * d.mcux);
    }
    int p0 = o->dc[0], p1 = o->dc[1], p2 = o->dc[2];      // scalars, not o->dc[c]: an indexed array would live in scratch
    int64_t at = entry >> 3;
    for (;;) {
        if (br.marker && br.nbits <= br.fake) at = d.scan_end * 8;
        else if (br.pos * 8 >= end_bits) at = br.bit_position();      // near the end of the chunk: the exact position
        else at = 0;                                                  // before it: position <= 8 * pos < end_bits
        if (at >= end_bits || (WRITE && first + n >= g.nblocks)) break;
        const int c = b < ny ? 0 : b - ny + 1;
        int pred = c == 0 ? p0 : (c == 1 ? p1 : p2);
        if (WRITE) {
            int64_t bi;
            if (c == 0) bi = (int64_t)(my * d.vs + (b >> (d.hs - 1))) * g.bw0 + mx * d.hs + (b & (d.hs - 1));
            else bi = (c == 1 ? g.off1 : g.off2) + (int64_t)my * d.mcux + mx;
            int16_t* out = blk(bi);
            jpg::decode_block(br, dt + 2 * c, dt + 2 * c + 1, pred, [&](int k, int v) { out[nat[k]] = (int16_t)v; });
            done(bi);
        } else {
            jpg::decode_block(br, dt + 2 * c, dt + 2 * c + 1, pred, [](int, int) {});
        }
        if (c == 0) p0 = pred; else if (c == 1) p1 = pred; else p2 = pred;
        ++n;
        if (++b == per_mcu) {
            b = 0;
            if (++mx == d.mcux) { mx = 0; ++my; }
        }
    }
    o->exit = chunk_state(at, b);
    o->nown = n;
    o->dc[0] = p0;
    o->dc[1] = p1;
    o->dc[2] = p2;
    o->status = br.status;
}

// IDCT of block `bi` of an image: coef (dequantised by q, natural order) -> 8x8 samples of its plane
JPG_HD void plane_of_block(const hirest_jpeg_image& d, const Geo& g, int64_t bi, int* comp, int64_t* off, int* pitch) {
    int c = 0;
    int64_t local = bi, base = 0;
    int bw = g.bw0;
    if (bi >= g.off2) { c = 2; local = bi - g.off2; base = g.off2; bw = d.mcux; }
    else if (bi >= g.off1) { c = 1; local = bi - g.off1; base = g.off1; bw = d.mcux; }
    const int64_t by = local / bw, bx = local - by * bw;
    *comp = c;
    *pitch = bw * 8;
    *off = base * 64 + by * 8 * (int64_t)(bw * 8) + bx * 8;
}

// RGB of output pixel (x, y) from the planes
struct PlaneReader {
    const uint8_t* p;
    int pitch;
    JPG_HD int operator()(int r, int c) const { return p[(int64_t)r * pitch + c]; }
};

JPG_HD uint32_t rgb_at(const hirest_jpeg_image& d, const PlaneReader& Y, const PlaneReader& Cb, const PlaneReader& Cr,
                       int cw, int ch, int x, int y) {
    const int yy = Y(y, x);
    if (d.ncomp == 1) return (uint32_t)yy * 0x010101u;
    return jpg::ycc_rgb(yy, jpg::chroma_at(Cb, x, y, d.hs, d.vs, cw, ch), jpg::chroma_at(Cr, x, y, d.hs, d.vs, cw, ch));
}

JPG_HD void planes_of(const hirest_jpeg_image& d, const uint8_t* planes, PlaneReader* Y, PlaneReader* Cb, PlaneReader* Cr, int* cw, int* ch) {
    const Geo g = geo_of(d);
    *Y = PlaneReader{planes, g.bw0 * 8};
    *Cb = PlaneReader{planes + g.off1 * 64, d.mcux * 8};
    *Cr = PlaneReader{planes + g.off2 * 64, d.mcux * 8};
    *cw = (d.width + d.hs - 1) / d.hs;
    *ch = (d.height + d.vs - 1) / d.vs;
}

// ------------------------------------------------------------------ host parse
inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

struct RawHuff {
    uint8_t bits[16], vals[256];
    bool defined, valid_ac, valid_dc;
};

bool huff_valid(const uint8_t* bits, int* nsym) {
    int code = 0, n = 0;
    for (int l = 1; l <= 16; ++l) {
        code += bits[l - 1];
        n += bits[l - 1];
        if (bits[l - 1] && code >= (1 << l)) return false;   // jpeg_make_d_derived_tbl: all-ones codes are rejected
        code <<= 1;
    }
    *nsym = n;
    return n <= 256;
}

int parse(const uint8_t* p, int64_t n, hirest_jpeg_image* img, hirest_jpeg_tables* tab) {
    memset(img, 0, sizeof(*img));
    memset(tab, 0, sizeof(*tab));
    auto fail = [&](int reason) { img->supported = 0; img->reason = reason; return 0; };
    if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return fail(HIREST_JPEG_NOT_JPEG);
    uint16_t qt[4][64];
    bool qdef[4] = {};
    RawHuff hf[2][4];
    for (auto& a : hf) for (auto& h : a) h.defined = false;
    const uint8_t nat[64] = JPG_NATURAL_ORDER;
    bool sof = false, jfif = false, adobe = false;
    int adobe_transform = -1, ri = 0;
    int nf = 0, cid[4] = {}, ch[4] = {}, cv[4] = {}, ctq[4] = {};
    int64_t pos = 2;
    for (;;) {
        if (pos >= n) return fail(HIREST_JPEG_TRUNCATED);
        if (p[pos] != 0xFF) return fail(HIREST_JPEG_NOT_JPEG);
        while (pos < n && p[pos] == 0xFF) ++pos;
        if (pos >= n) return fail(HIREST_JPEG_TRUNCATED);
        const int m = p[pos++];
        if (m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) return fail(HIREST_JPEG_NOT_JPEG);
        if (pos + 2 > n) return fail(HIREST_JPEG_TRUNCATED);
        const int len = be16(p + pos);
        if (len < 2) return fail(HIREST_JPEG_NOT_JPEG);
        if (pos + len > n) return fail(HIREST_JPEG_TRUNCATED);
        const uint8_t* s = p + pos + 2;
        const int sl = len - 2;
        const int64_t next = pos + len;
        if (m == 0xC2 || m == 0xC6) return fail(HIREST_JPEG_PROGRESSIVE);
        if (m == 0xC3 || m == 0xC5 || m == 0xC7) return fail(HIREST_JPEG_LOSSLESS);
        if (m == 0xCC || (m >= 0xC9 && m <= 0xCB) || m >= 0xCD && m <= 0xCF) return fail(HIREST_JPEG_ARITHMETIC);
        if (m == 0xC0 || m == 0xC1) {
            if (sof || sl < 6) return fail(HIREST_JPEG_NOT_JPEG);
            if (s[0] != 8) return fail(HIREST_JPEG_PRECISION);
            img->height = be16(s + 1);
            img->width = be16(s + 3);
            nf = s[5];
            if (sl < 6 + 3 * nf || nf < 1) return fail(HIREST_JPEG_NOT_JPEG);
            if (nf != 1 && nf != 3) return fail(HIREST_JPEG_COLOR);
            for (int i = 0; i < nf; ++i) {
                cid[i] = s[6 + 3 * i];
                ch[i] = s[7 + 3 * i] >> 4;
                cv[i] = s[7 + 3 * i] & 15;
                ctq[i] = s[8 + 3 * i];
                if (ch[i] < 1 || ch[i] > 4 || cv[i] < 1 || cv[i] > 4 || ctq[i] > 3) return fail(HIREST_JPEG_NOT_JPEG);
            }
            if (img->width < 1 || img->height < 1) return fail(HIREST_JPEG_SIZE);   // 0 = height from DNL
            if (img->width > MAX_DIM || img->height > MAX_DIM) return fail(HIREST_JPEG_SIZE);
            sof = true;
        } else if (m == 0xC4) {
            int o = 0;
            while (o < sl) {
                if (o + 17 > sl) return fail(HIREST_JPEG_NOT_JPEG);
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) return fail(HIREST_JPEG_NOT_JPEG);
                RawHuff& h = hf[tc][th];
                memcpy(h.bits, s + o + 1, 16);
                int nsym = 0;
                for (int l = 0; l < 16; ++l) nsym += h.bits[l];
                if (nsym > 256 || o + 17 + nsym > sl) return fail(HIREST_JPEG_NOT_JPEG);
                memset(h.vals, 0, 256);
                memcpy(h.vals, s + o + 17, nsym);
                int ns2 = 0;
                h.defined = true;
                h.valid_ac = huff_valid(h.bits, &ns2);
                h.valid_dc = h.valid_ac;
                for (int i = 0; i < nsym; ++i) if (h.vals[i] > 15) h.valid_dc = false;
                o += 17 + nsym;
            }
        } else if (m == 0xDB) {
            int o = 0;
            while (o < sl) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (pq > 1 || tq > 3 || o + 1 + 64 * (pq + 1) > sl) return fail(HIREST_JPEG_NOT_JPEG);
                for (int k = 0; k < 64; ++k)
                    qt[tq][nat[k]] = pq ? (uint16_t)be16(s + o + 1 + 2 * k) : s[o + 1 + k];
                qdef[tq] = true;
                o += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xDD) {
            if (sl < 2) return fail(HIREST_JPEG_NOT_JPEG);
            ri = be16(s);
        } else if (m == 0xE0) {
            if (sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
        } else if (m == 0xDA) {
            if (!sof || sl < 1) return fail(HIREST_JPEG_NOT_JPEG);
            const int ns = s[0];
            if (sl < 4 + 2 * ns) return fail(HIREST_JPEG_NOT_JPEG);
            if (ns != nf) return fail(HIREST_JPEG_MULTI_SCAN);
            const int ss = s[1 + 2 * ns], se = s[2 + 2 * ns], ahal = s[3 + 2 * ns];
            if (ss != 0 || se != 63 || ahal != 0) return fail(HIREST_JPEG_NOT_JPEG);
            // colour space as libjpeg guesses it (jdapimin.c default_decompress_parms)
            if (nf == 3) {
                if (!jfif && adobe && adobe_transform == 0) return fail(HIREST_JPEG_COLOR);
                if (!jfif && !adobe && cid[0] == 82 && cid[1] == 71 && cid[2] == 66) return fail(HIREST_JPEG_COLOR);
                const bool ok = ch[1] == 1 && cv[1] == 1 && ch[2] == 1 && cv[2] == 1 &&
                                ((ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2));
                if (!ok) return fail(HIREST_JPEG_SAMPLING);
                img->hs = ch[0];
                img->vs = cv[0];
            } else {
                img->hs = img->vs = 1;   // a single-component scan is non-interleaved: one block per MCU
            }
            for (int i = 0; i < ns; ++i) {
                if (s[1 + 2 * i] != cid[i]) return fail(HIREST_JPEG_MULTI_SCAN);
                const int td = s[2 + 2 * i] >> 4, ta = s[2 + 2 * i] & 15;
                if (td > 3 || ta > 3) return fail(HIREST_JPEG_NOT_JPEG);
                const RawHuff &hd = hf[0][td], &ha = hf[1][ta];
                if (!hd.defined || !ha.defined || !hd.valid_dc || !ha.valid_ac || !qdef[ctq[i]]) return fail(HIREST_JPEG_BAD_TABLES);
                memcpy(tab->qt[i], qt[ctq[i]], sizeof(tab->qt[i]));
                memcpy(tab->huff_bits[2 * i], hd.bits, 16);
                memcpy(tab->huff_vals[2 * i], hd.vals, 256);
                memcpy(tab->huff_bits[2 * i + 1], ha.bits, 16);
                memcpy(tab->huff_vals[2 * i + 1], ha.vals, 256);
            }
            img->ncomp = nf;
            img->restart_interval = ri;
            img->mcux = (img->width + 8 * img->hs - 1) / (8 * img->hs);
            img->mcuy = (img->height + 8 * img->vs - 1) / (8 * img->vs);
            img->scan_begin = next;
            // the scan ends at the first marker that is not RSTn; it must be EOI
            int64_t q = next;
            for (;;) {
                const void* f = q < n ? memchr(p + q, 0xFF, (size_t)(n - q)) : nullptr;
                if (!f) return fail(HIREST_JPEG_TRUNCATED);
                const int64_t at = (const uint8_t*)f - p;
                int64_t r = at + 1;
                while (r < n && p[r] == 0xFF) ++r;
                if (r >= n) return fail(HIREST_JPEG_TRUNCATED);
                if (p[r] == 0 || (p[r] >= 0xD0 && p[r] <= 0xD7)) { q = r + 1; continue; }
                if (p[r] != 0xD9) return fail(HIREST_JPEG_MULTI_SCAN);
                img->scan_end = at;
                break;
            }
            img->supported = 1;
            img->reason = HIREST_JPEG_OK;
            return 0;
        } else if (m == 0xDC) {
            return fail(HIREST_JPEG_NOT_JPEG);
        }
        pos = next;
    }
}

void host_dtables(const hirest_jpeg_tables* t, jpg::DTable* dt) {
    for (int i = 0; i < 6; ++i) {
        jpg::build_dtable(t->huff_bits[i], t->huff_vals[i], dt + i);
        for (int v = 0; v < 256; ++v) dt[i].look[v] = jpg::look_entry(dt + i, v);
    }
}

// ------------------------------------------------------------------ kernels
// One lane per image.  RESTART_ONLY (the chunked entry's launch for what its own kernel leaves alone): images without a restart
// interval are skipped.
template <bool RESTART_ONLY>
__device__ __forceinline__ void entropy_lanes(const hirest_jpeg_image* __restrict__ imgs, int32_t first, int32_t count,
                                              const hirest_jpeg_tables* __restrict__ tables, int32_t set,
                                              const uint8_t* __restrict__ data, uint8_t* __restrict__ ws,
                                              int32_t* __restrict__ status) {
    __shared__ jpg::DTable dt[6];
    __shared__ uint8_t nat[64];
    // each lane assembles its current block here and stores it with 8 x 16 B: scattered 2-byte global stores would make
    // every later load wait for them (gfx9's vmcnt counts stores too)
    __shared__ alignas(16) int16_t bb[ENT_LANES][64];
    const int t = threadIdx.x;
    const hirest_jpeg_tables* tb = tables + set;
    if (t < 6) jpg::build_dtable(tb->huff_bits[t], tb->huff_vals[t], dt + t);
    for (int k = t; k < 64; k += ENT_LANES) nat[k] = kNatural[k];
    __syncthreads();
    for (int e = t; e < 6 * 256; e += ENT_LANES) dt[e >> 8].look[e & 255] = jpg::look_entry(dt + (e >> 8), e & 255);
    __syncthreads();
    const int i = blockIdx.x * ENT_LANES + t;
    if (i >= count) return;
    const hirest_jpeg_image d = imgs[first + i];
    if (!d.supported) {
        status[first + i] = JPG_ST_UNSUPPORTED;
        return;
    }
    if (RESTART_ONLY && d.restart_interval == 0) return;
    int16_t* coef = (int16_t*)(ws + d.ws_offset);
    uint4* mine = (uint4*)bb[t];
    const int st = decode_scan(
        d, data + d.data_offset, dt, nat,
        [&](int64_t) {
            const uint4 z = make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 8; ++j) mine[j] = z;
            return bb[t];
        },
        [&](int64_t bi) {
            uint4* g = (uint4*)(coef + bi * COEF_STRIDE);
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = mine[j];
        });
    status[first + i] = st;
}

__global__ void __launch_bounds__(ENT_LANES) jpeg_entropy_kernel(const hirest_jpeg_image* __restrict__ imgs, int32_t first, int32_t count,
                                                                 const hirest_jpeg_tables* __restrict__ tables, int32_t set,
                                                                 const uint8_t* __restrict__ data, uint8_t* __restrict__ ws,
                                                                 int32_t* __restrict__ status) {
    entropy_lanes<false>(imgs, first, count, tables, set, data, ws, status);
}

__global__ void __launch_bounds__(ENT_LANES) jpeg_entropy_restart_kernel(const hirest_jpeg_image* __restrict__ imgs, int32_t first, int32_t count,
                                                                         const hirest_jpeg_tables* __restrict__ tables, int32_t set,
                                                                         const uint8_t* __restrict__ data, uint8_t* __restrict__ ws,
                                                                         int32_t* __restrict__ status) {
    entropy_lanes<true>(imgs, first, count, tables, set, data, ws, status);
}

// One workgroup per image of the run [first, first + gridDim.x), one lane per chunk (blockDim.x = the most lanes any image of
// the run needs).  Exits and the scan go through LDS behind barriers; every lane stages its current block in LDS and stores it
// whole, as jpeg_entropy_kernel does.  Images with a restart interval and unsupported ones are jpeg_entropy_restart_kernel's.
// info[4 i ..]: chunk bytes, lanes, sync rounds, blocks found (capped) of image i.
__global__ void __launch_bounds__(CHUNK_MAX_LANES) jpeg_entropy_chunked_kernel(const hirest_jpeg_image* __restrict__ imgs, int32_t first,
                                                                               const hirest_jpeg_tables* __restrict__ tables, int32_t set,
                                                                               const uint8_t* __restrict__ data, uint8_t* __restrict__ ws,
                                                                               int32_t* __restrict__ status, int64_t chunk_bytes,
                                                                               int32_t* __restrict__ info) {
    __shared__ jpg::DTable dt[6];
    __shared__ uint8_t nat[64];
    __shared__ int32_t st_or;
    // blockDim.x * 128 B: first the lanes' exits (8 B each) and the two scan buffers (16 B each), then the staged blocks
    extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
    const int t = threadIdx.x, T = blockDim.x;
    const int i = first + blockIdx.x;
    const hirest_jpeg_image d = imgs[i];
    if (!d.supported || d.restart_interval != 0) return;          // uniform
    const hirest_jpeg_tables* tb = tables + set;
    if (t < 6) jpg::build_dtable(tb->huff_bits[t], tb->huff_vals[t], dt + t);
    if (t < 64) nat[t] = kNatural[t];
    if (t == 0) st_or = 0;
    __syncthreads();
    for (int e = t; e < 6 * 256; e += T) dt[e >> 8].look[e & 255] = jpg::look_entry(dt + (e >> 8), e & 255);
    __syncthreads();
    const Geo g = geo_of(d);
    const uint8_t* file = data + d.data_offset;
    const int64_t len = d.scan_end - d.scan_begin;
    const int64_t cb = chunk_size(len, chunk_bytes, CHUNK_MAX_LANES);
    const int lanes = (int)((len + cb - 1) / cb);                 // <= blockDim.x: the host sized the launch with the same rule
    const int64_t end_bits = (t + 1 >= lanes ? d.scan_end : d.scan_begin + (int64_t)(t + 1) * cb) * 8;
    int64_t* exits = (int64_t*)dyn;
    auto none = [](int64_t) { return (int16_t*)nullptr; };
    auto nop = [](int64_t) {};
    // sync pass
    int64_t entry = 0;
    if (t < lanes) entry = t == 0 ? chunk_state(d.scan_begin * 8, 0) : chunk_guess(d, file, cb, t);
    ChunkOut rec{};
    bool need = t < lanes;
    int rounds = 0;
    for (int r = 0; r < lanes; ++r) {
        if (!__syncthreads_or(need)) break;
        ++rounds;
        if (need) {
            rec = ChunkOut{};
            decode_chunk<false>(d, g, file, dt, nat, entry, end_bits, 0, &rec, none, nop);
            exits[t] = rec.exit;
        }
        __syncthreads();
        need = false;
        if (t > 0 && t < lanes && exits[t - 1] != entry) {
            entry = exits[t - 1];
            need = true;
        }
    }
    // exclusive scan over the lanes: first block and predictors of each
    int4* sc = (int4*)(dyn + 8 * (size_t)T);
    int4 own = t < lanes ? make_int4(rec.nown, rec.dc[0], rec.dc[1], rec.dc[2]) : make_int4(0, 0, 0, 0);
    int4 acc = own;
    int cur = 0;
    sc[t] = acc;
    __syncthreads();
    for (int o = 1; o < T; o <<= 1) {
        if (t >= o) {
            const int4 v = sc[cur * T + t - o];
            // unsigned: garbage can make the sums wrap, and the wrapped value is what the serial predictor holds too
            acc = make_int4((int)((unsigned)acc.x + (unsigned)v.x), (int)((unsigned)acc.y + (unsigned)v.y),
                            (int)((unsigned)acc.z + (unsigned)v.z), (int)((unsigned)acc.w + (unsigned)v.w));
        }
        cur ^= 1;
        sc[cur * T + t] = acc;
        __syncthreads();
    }
    const int found = sc[cur * T + T - 1].x;
    __syncthreads();                                              // the staged blocks reuse this LDS
    // write pass
    if (t < lanes) {
        int16_t* bb = (int16_t*)(dyn + 128 * (size_t)t);
        uint4* mine = (uint4*)bb;
        int16_t* coef = (int16_t*)(ws + d.ws_offset);
        ChunkOut w{};
        w.dc[0] = (int)((unsigned)acc.y - (unsigned)own.y);
        w.dc[1] = (int)((unsigned)acc.z - (unsigned)own.z);
        w.dc[2] = (int)((unsigned)acc.w - (unsigned)own.w);
        decode_chunk<true>(
            d, g, file, dt, nat, entry, end_bits, (int64_t)(acc.x - own.x), &w,
            [&](int64_t) {
                const uint4 z = make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 8; ++j) mine[j] = z;
                return bb;
            },
            [&](int64_t bi) {
                uint4* go = (uint4*)(coef + bi * COEF_STRIDE);
#pragma unroll
                for (int j = 0; j < 8; ++j) go[j] = mine[j];
            });
        if (w.status) atomicOr(&st_or, w.status);
    }
    __syncthreads();
    if (t == 0) {
        status[i] = st_or | (found < g.nblocks ? JPG_ST_OUT_OF_DATA : 0);      // fewer blocks than the image has: the data ran out
        info[4 * i] = (int32_t)cb;
        info[4 * i + 1] = lanes;
        info[4 * i + 2] = rounds;
        info[4 * i + 3] = found;
    }
}

__global__ void __launch_bounds__(IDCT_BLOCKS * 8) jpeg_idct_kernel(const hirest_jpeg_image* __restrict__ imgs,
                                                                     const hirest_jpeg_tables* __restrict__ tables,
                                                                     uint8_t* __restrict__ ws, const int32_t* __restrict__ status) {
    __shared__ alignas(16) int16_t cf[IDCT_BLOCKS][64];
    __shared__ int32_t wk[IDCT_BLOCKS][65];
    const int img = blockIdx.y;
    if (status[img] != 0) return;                      // uniform: unsupported or failed images are the fallback's
    const hirest_jpeg_image d = imgs[img];
    const Geo g = geo_of(d);
    const int t = threadIdx.x, lb = t >> 3, r = t & 7;
    const int64_t bi = (int64_t)blockIdx.x * IDCT_BLOCKS + lb;
    if ((int64_t)blockIdx.x * IDCT_BLOCKS >= g.nblocks) return;   // uniform
    const bool valid = bi < g.nblocks;
    const int16_t* coef = (const int16_t*)(ws + d.ws_offset);
    if (valid) *(uint4*)&cf[lb][r * 8] = *(const uint4*)(coef + bi * COEF_STRIDE + r * 8);
    __syncthreads();
    int comp = 0, pitch = 0;
    int64_t off = 0;
    if (valid) {
        plane_of_block(d, g, bi, &comp, &off, &pitch);
        const uint16_t* q = tables[d.table_set].qt[comp];
        int32_t col[8], w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) col[k] = (int32_t)cf[lb][k * 8 + r] * (int32_t)q[k * 8 + r];
        jpg::idct_col(col, w);
#pragma unroll
        for (int k = 0; k < 8; ++k) wk[lb][k * 8 + r] = w[k];
    }
    __syncthreads();
    if (valid) {
        int32_t row[8];
        uint8_t o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) row[k] = wk[lb][r * 8 + k];
        jpg::idct_row(row, o);
        uint2 v;
        v.x = o[0] | (o[1] << 8) | (o[2] << 16) | ((uint32_t)o[3] << 24);
        v.y = o[4] | (o[5] << 8) | (o[6] << 16) | ((uint32_t)o[7] << 24);
        *(uint2*)(ws + d.plane_offset + off + (int64_t)r * pitch) = v;
    }
}

__global__ void __launch_bounds__(COLOR_THREADS) jpeg_color_kernel(const hirest_jpeg_image* __restrict__ imgs, const uint8_t* __restrict__ ws,
                                                                   uint8_t* __restrict__ out, const int32_t* __restrict__ status) {
    const int img = blockIdx.y;
    if (status[img] != 0) return;
    const hirest_jpeg_image d = imgs[img];
    const int cpr = (d.width + 15) >> 4;
    const int64_t chunk = (int64_t)blockIdx.x * COLOR_THREADS + threadIdx.x;
    if (chunk >= (int64_t)cpr * d.height) return;
    const int y = (int)(chunk / cpr), x0 = (int)(chunk - (int64_t)y * cpr) * 16;
    const uint8_t* planes = ws + d.plane_offset;
    PlaneReader Y, Cb, Cr;
    int cw, ch;
    planes_of(d, planes, &Y, &Cb, &Cr, &cw, &ch);
    uint8_t* dst = out + d.out_offset + ((int64_t)y * d.width + x0) * 3;
    if (x0 + 16 <= d.width && ((uintptr_t)dst & 15) == 0) {
        uint32_t w[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) w[j] = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t px = rgb_at(d, Y, Cb, Cr, cw, ch, x0 + i, y);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int pb = 3 * i + k;
                w[pb >> 2] |= ((px >> (8 * k)) & 255u) << (8 * (pb & 3));
            }
        }
        uint4* o = (uint4*)dst;
        o[0] = make_uint4(w[0], w[1], w[2], w[3]);
        o[1] = make_uint4(w[4], w[5], w[6], w[7]);
        o[2] = make_uint4(w[8], w[9], w[10], w[11]);
    } else {
        for (int i = 0; i < 16 && x0 + i < d.width; ++i) {
            const uint32_t px = rgb_at(d, Y, Cb, Cr, cw, ch, x0 + i, y);
            dst[3 * i] = px & 255;
            dst[3 * i + 1] = (px >> 8) & 255;
            dst[3 * i + 2] = (px >> 16) & 255;
        }
    }
}

}  // namespace

extern "C" int hirest_jpeg_parse(const uint8_t* data, int64_t size, hirest_jpeg_image* img, hirest_jpeg_tables* tables) {
    if (!data || size < 0 || !img || !tables) return HIREST_E_BADARG;
    return parse(data, size, img, tables);
}

extern "C" int64_t hirest_jpeg_workspace_bytes(hirest_jpeg_image* imgs, int32_t n) {
    if (n < 0 || (n > 0 && !imgs)) return HIREST_E_BADARG;
    int64_t total = 0;
    // coefficients: the entropy launches' groups (runs of one table set, 64 images per workgroup), lanes interleaved
    for (int i = 0; i < n;) {
        int j = i + 1;
        while (j < n && imgs[j].table_set == imgs[i].table_set) ++j;
        for (int g0 = i; g0 < j; g0 += ENT_LANES) {
            const int g1 = g0 + ENT_LANES < j ? g0 + ENT_LANES : j;
            int64_t maxb = 0;
            for (int k = g0; k < g1; ++k) {
                imgs[k].ws_offset = total + (int64_t)(k - g0) * 128;
                if (imgs[k].supported && geo_of(imgs[k]).nblocks > maxb) maxb = geo_of(imgs[k]).nblocks;
            }
            total += align256(maxb * COEF_STRIDE * 2);
        }
        i = j;
    }
    for (int k = 0; k < n; ++k) {   // component planes, one run per image
        imgs[k].plane_offset = total;
        if (imgs[k].supported) total += align256(geo_of(imgs[k]).nblocks * 64);
    }
    return total;
}

// IDCT, upsampling and colour of one image on the CPU: coef = nblocks x 64 int16 in component-plane block order
static void host_pixels(const hirest_jpeg_image& d, const hirest_jpeg_tables* tables, const std::vector<int16_t>& coef, uint8_t* out) {
    const Geo g = geo_of(d);
    std::vector<uint8_t> planes((size_t)g.nblocks * 64);
    for (int64_t bi = 0; bi < g.nblocks; ++bi) {
        int comp, pitch;
        int64_t off;
        plane_of_block(d, g, bi, &comp, &off, &pitch);
        const int16_t* c = coef.data() + bi * 64;
        const uint16_t* q = tables->qt[comp];
        int32_t wk[64];
        for (int col = 0; col < 8; ++col) {
            int32_t in[8], w[8];
            for (int k = 0; k < 8; ++k) in[k] = (int32_t)c[k * 8 + col] * (int32_t)q[k * 8 + col];
            jpg::idct_col(in, w);
            for (int k = 0; k < 8; ++k) wk[k * 8 + col] = w[k];
        }
        for (int r = 0; r < 8; ++r) jpg::idct_row(wk + r * 8, planes.data() + off + (int64_t)r * pitch);
    }
    PlaneReader Y, Cb, Cr;
    int cw, ch;
    planes_of(d, planes.data(), &Y, &Cb, &Cr, &cw, &ch);
    for (int y = 0; y < d.height; ++y)
        for (int x = 0; x < d.width; ++x) {
            const uint32_t px = rgb_at(d, Y, Cb, Cr, cw, ch, x, y);
            uint8_t* o = out + ((int64_t)y * d.width + x) * 3;
            o[0] = px & 255;
            o[1] = (px >> 8) & 255;
            o[2] = (px >> 16) & 255;
        }
}

extern "C" int hirest_jpeg_decode_host(const hirest_jpeg_image* img, const hirest_jpeg_tables* tables, const uint8_t* data,
                                       uint8_t* out, int32_t* status) {
    if (!img || !tables || !data || !out || !status) return HIREST_E_BADARG;
    const hirest_jpeg_image& d = *img;
    if (!d.supported) {
        *status = JPG_ST_UNSUPPORTED;
        return 0;
    }
    const Geo g = geo_of(d);
    jpg::DTable dt[6];
    host_dtables(tables, dt);
    const uint8_t nat[64] = JPG_NATURAL_ORDER;
    std::vector<int16_t> coef((size_t)g.nblocks * 64);
    const int st = decode_scan(
        d, data, dt, nat,
        [&](int64_t bi) {
            int16_t* b = coef.data() + bi * 64;
            memset(b, 0, 128);
            return b;
        },
        [](int64_t) {});
    *status = st;
    if (st) return 0;
    host_pixels(d, tables, coef, out);
    return 0;
}

// The chunked decode with the lanes run one after another: the same rounds as jpeg_entropy_chunked_kernel (every lane of a
// round sees its neighbour's exit of the round before), so `rounds_out` is the device's count too.
extern "C" int hirest_jpeg_decode_host_chunked(const hirest_jpeg_image* img, const hirest_jpeg_tables* tables, const uint8_t* data,
                                               int64_t chunk_bytes, uint8_t* out, int32_t* status, int32_t* rounds_out) {
    if (!img || !tables || !data || !out || !status || chunk_bytes < 0) return HIREST_E_BADARG;
    const hirest_jpeg_image& d = *img;
    if (rounds_out) *rounds_out = 0;
    if (!d.supported) {
        *status = JPG_ST_UNSUPPORTED;
        return 0;
    }
    if (d.restart_interval != 0 || d.scan_end <= d.scan_begin) return HIREST_E_BADARG;   // restart intervals: hirest_jpeg_decode_host
    const Geo g = geo_of(d);
    jpg::DTable dt[6];
    host_dtables(tables, dt);
    const uint8_t nat[64] = JPG_NATURAL_ORDER;
    const int64_t len = d.scan_end - d.scan_begin;
    const int64_t cb = chunk_size(len, chunk_bytes, chunk_bytes > 0 ? len : CHUNK_MAX_LANES);   // a given size is kept as it is
    const int64_t lanes = (len + cb - 1) / cb;
    auto end_bits = [&](int64_t l) { return (l + 1 == lanes ? d.scan_end : d.scan_begin + (l + 1) * cb) * 8; };
    auto none = [](int64_t) { return (int16_t*)nullptr; };
    auto nop = [](int64_t) {};
    std::vector<int64_t> entry(lanes), prev_exit(lanes);
    std::vector<ChunkOut> rec(lanes);
    int rounds = 0;
    for (int64_t r = 0; r < lanes; ++r) {
        for (int64_t l = 0; l < lanes; ++l) prev_exit[l] = rec[l].exit;
        bool any = false;
        for (int64_t l = 0; l < lanes; ++l) {
            const int64_t e = r == 0 ? (l == 0 ? chunk_state(d.scan_begin * 8, 0) : chunk_guess(d, data, cb, l)) : (l == 0 ? entry[0] : prev_exit[l - 1]);
            if (r > 0 && e == entry[l]) continue;
            any = true;
            entry[l] = e;
            rec[l] = ChunkOut{};
            decode_chunk<false>(d, g, data, dt, nat, e, end_bits(l), 0, &rec[l], none, nop);
        }
        if (!any) break;
        ++rounds;
    }
    if (rounds_out) *rounds_out = rounds;
    std::vector<int16_t> coef((size_t)g.nblocks * 64);
    int st = 0;
    int64_t first = 0;
    int32_t pred[3] = {0, 0, 0};
    for (int64_t l = 0; l < lanes; ++l) {
        ChunkOut w{};
        for (int c = 0; c < 3; ++c) w.dc[c] = pred[c];
        decode_chunk<true>(
            d, g, data, dt, nat, entry[l], end_bits(l), first, &w,
            [&](int64_t bi) {
                int16_t* b = coef.data() + bi * 64;
                memset(b, 0, 128);
                return b;
            },
            nop);
        st |= w.status;
        first += rec[l].nown;
        for (int c = 0; c < 3; ++c) pred[c] += rec[l].dc[c];
    }
    if (first < g.nblocks) st |= JPG_ST_OUT_OF_DATA;      // the data ended before the image did
    *status = st;
    if (st) return 0;
    host_pixels(d, tables, coef, out);
    return 0;
}

// argument checks of the device entries; max_blocks / max_chunks size the IDCT and colour launches
static int check_images(const hirest_jpeg_image* imgs_host, const hirest_jpeg_image* imgs_dev, int32_t n, const hirest_jpeg_tables* tables_dev,
                        const uint8_t* data, uint8_t* out, int32_t* status, void* workspace, int64_t workspace_bytes, int64_t* max_blocks,
                        int64_t* max_chunks) {
    if (!imgs_host || !imgs_dev || !tables_dev || !data || !out || !status || n < 0 || n > 65535) return HIREST_E_BADARG;
    if (((uintptr_t)workspace & 255) != 0 || ((uintptr_t)data & 7) != 0) return HIREST_E_BADARG;
    *max_blocks = *max_chunks = 0;
    for (int i = 0; i < n; ++i) {
        const hirest_jpeg_image& d = imgs_host[i];
        if (!d.supported) continue;
        const Geo g = geo_of(d);
        if (d.ws_offset < 0 || (d.ws_offset & 127) || d.ws_offset + (g.nblocks - 1) * COEF_STRIDE * 2 + 128 > workspace_bytes ||
            d.plane_offset < 0 || (d.plane_offset & 255) || d.plane_offset + g.nblocks * 64 > workspace_bytes)
            return HIREST_E_WORKSPACE;
        if (d.table_set < 0 || d.data_offset < 0 || (d.data_offset & 7) || d.out_offset < 0 || d.scan_begin < 0 ||
            d.scan_end <= d.scan_begin)
            return HIREST_E_BADARG;
        *max_blocks = g.nblocks > *max_blocks ? g.nblocks : *max_blocks;
        const int64_t ch = (int64_t)((d.width + 15) >> 4) * d.height;
        *max_chunks = ch > *max_chunks ? ch : *max_chunks;
    }
    return 0;
}

// coefficients -> frames of the images whose status is 0
static int launch_pixels(const hirest_jpeg_image* imgs_dev, int32_t n, const hirest_jpeg_tables* tables_dev, uint8_t* out, int32_t* status,
                         void* workspace, int64_t max_blocks, int64_t max_chunks, hipStream_t s) {
    if (max_blocks == 0) return hirest_launch_status();
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS), n), dim3(IDCT_BLOCKS * 8), 0, s,
                       imgs_dev, tables_dev, (uint8_t*)workspace, (const int32_t*)status);
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((max_chunks + COLOR_THREADS - 1) / COLOR_THREADS), n), dim3(COLOR_THREADS), 0, s,
                       imgs_dev, (const uint8_t*)workspace, out, (const int32_t*)status);
    return hirest_launch_status();
}

extern "C" int hirest_jpeg_decode(const hirest_jpeg_image* imgs_host, const hirest_jpeg_image* imgs_dev, int32_t n,
                                  const hirest_jpeg_tables* tables_dev, const uint8_t* data, uint8_t* out, int32_t* status,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    if (n == 0) return 0;
    int64_t max_blocks = 0, max_chunks = 0;
    const int rc = check_images(imgs_host, imgs_dev, n, tables_dev, data, out, status, workspace, workspace_bytes, &max_blocks, &max_chunks);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    // entropy decode: one launch per run of images sharing a table set (the caller groups them)
    for (int i = 0; i < n;) {
        int j = i + 1;
        while (j < n && imgs_host[j].table_set == imgs_host[i].table_set) ++j;
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((j - i + ENT_LANES - 1) / ENT_LANES), dim3(ENT_LANES), 0, s, imgs_dev, i, j - i,
                           tables_dev, imgs_host[i].table_set, data, (uint8_t*)workspace, status);
        i = j;
    }
    return launch_pixels(imgs_dev, n, tables_dev, out, status, workspace, max_blocks, max_chunks, s);
}

extern "C" int64_t hirest_jpeg_chunked_workspace_bytes(int32_t n) {
    if (n < 0) return HIREST_E_BADARG;
    return align256((int64_t)n * 16);
}

extern "C" int hirest_jpeg_decode_chunked(const hirest_jpeg_image* imgs_host, const hirest_jpeg_image* imgs_dev, int32_t n,
                                          const hirest_jpeg_tables* tables_dev, const uint8_t* data, uint8_t* out, int32_t* status,
                                          void* workspace, int64_t workspace_bytes, int64_t chunk_bytes, void* chunk_workspace,
                                          int64_t chunk_workspace_bytes, void* stream) {
    if (n == 0) return 0;
    int64_t max_blocks = 0, max_chunks = 0;
    const int rc = check_images(imgs_host, imgs_dev, n, tables_dev, data, out, status, workspace, workspace_bytes, &max_blocks, &max_chunks);
    if (rc) return rc;
    if (chunk_bytes < 0 || !chunk_workspace || ((uintptr_t)chunk_workspace & 15) != 0) return HIREST_E_BADARG;
    if (chunk_workspace_bytes < hirest_jpeg_chunked_workspace_bytes(n)) return HIREST_E_WORKSPACE;
    static HirestDevCfg cfg;
    const int rc2 = hirest_configure(jpeg_entropy_chunked_kernel, CHUNK_MAX_LANES * 128, cfg);
    if (rc2) return rc2;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t me = hipMemsetAsync(chunk_workspace, 0, (size_t)n * 16, s);   // images the chunked kernel does not decode: all zero
    if (me != hipSuccess) return (int)me;
    for (int i = 0; i < n;) {
        int j = i + 1;
        while (j < n && imgs_host[j].table_set == imgs_host[i].table_set) ++j;
        int64_t lanes = 0;
        bool others = false;            // unsupported images (status only) and restart intervals: one lane per image
        for (int k = i; k < j; ++k) {
            const hirest_jpeg_image& d = imgs_host[k];
            if (!d.supported || d.restart_interval != 0) {
                others = true;
                continue;
            }
            const int64_t len = d.scan_end - d.scan_begin, cb = chunk_size(len, chunk_bytes, CHUNK_MAX_LANES);
            const int64_t l = (len + cb - 1) / cb;
            lanes = l > lanes ? l : lanes;
        }
        if (lanes > 0) {
            const int threads = (int)((lanes + 63) / 64 * 64);
            hipLaunchKernelGGL(jpeg_entropy_chunked_kernel, dim3(j - i), dim3(threads), (size_t)threads * 128, s, imgs_dev, i, tables_dev,
                               imgs_host[i].table_set, data, (uint8_t*)workspace, status, chunk_bytes, (int32_t*)chunk_workspace);
        }
        if (others)
            hipLaunchKernelGGL(jpeg_entropy_restart_kernel, dim3((j - i + ENT_LANES - 1) / ENT_LANES), dim3(ENT_LANES), 0, s, imgs_dev, i, j - i,
                               tables_dev, imgs_host[i].table_set, data, (uint8_t*)workspace, status);
        i = j;
    }
    return launch_pixels(imgs_dev, n, tables_dev, out, status, workspace, max_blocks, max_chunks, s);
}
