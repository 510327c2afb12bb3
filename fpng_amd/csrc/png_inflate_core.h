// png_inflate_core.h -- the general decode tier's per-wave logic (png_inflate.hip, png_decode_api.cpp): ordinary PNG files, as
// libpng, Pillow or zlib write them.  One 64-lane wave works on one file: pngi_inflate walks the chunks, inflates the zlib stream
// that the IDAT chunks carry (RFC 1950 / 1951) into the file's filtered scanlines, pngi_unfilter undoes PNG filters 0-4 and
// expands the pixels; pngi_unfilter_box does the same for the rows and pixels that a box of the image needs and stores the box as
// tight uint8 planes, the layout the views stage reads (view_plan.h).  The same text compiles for the GPU (hipcc) and, with plain g++, for the host: there the wave's lanes run one
// after the other inside PNGI_LANES, a value every lane holds (PngiLane<T>) is an array of 64, the wave operation (pngi_shift_up)
// is a loop and the LDS arrays are plain arrays.  tests/cpp/png_inflate_host.cpp and png_unfilter_box_host.cpp run that form, under
// the sanitizers too.
//
// Rules of this tier (include/fpng_amd.h has the caller's view):
//   * 8-bit grey, grey + alpha, RGB, palette, RGBA; no interlace; any number of consecutive IDAT chunks, empty ones included.
//   * The whole zlib stream must be a valid deflate stream up to its final block's end-of-block symbol.  Output beyond the image's
//     h * (1 + bytes per row) bytes is inflated, checked and never stored; such a file is ACCEPTED, as Pillow 12 accepts it (its
//     decoder stops at the image's last row and never looks at what follows; a damaged stream behind the image, which Pillow
//     therefore lets pass, is refused here).
//   * The code length code must be complete.  The literal/length and the distance code may each be complete or consist of one
//     single 1-bit code, as zlib allows (RFC 1951 for distances; fpng writes it): for literal/length that is the end-of-block
//     symbol alone, a block without output.  The distance code may also have no code at all (a block of literals).  The unused
//     code of a single-code table is no code: meeting it is INVALID_IDAT.
//   * Chunk CRCs behind IHDR, the stream's Adler-32 and the presence of IEND are not checked.  The zlib window size is checked in
//     the header only: distances are held against the output so far and 32768.
//   * The box entry visits rows 0 .. y1 - 1 and of each row pixels 0 .. x1 - 1 (x1 = box.x + box.w, y1 = box.y + box.h): no predictor
//     reads to the right of or below a pixel.  INVALID_IDAT is a filter byte above 4 in one of those rows, or a palette index at or
//     behind PLTE's count at a pixel INSIDE the box; rows and pixels that are never visited cannot fail a file (the fpng tier's crop
//     calls have the same property), nor can a palette index outside the box.  The stream is inflated and checked to its end all
//     the same, and refused if it yields fewer than h * (1 + bytes per row) bytes: File::need_bytes.
//   * Every loop ends because it consumes input bits or file bytes, or produces output bytes: the file has at most 2^32 bytes, a
//     token at least one bit and at most 258 output bytes.  No workgroup waits for another one.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define PNGI_FN __device__ inline
#define PNGI_HD __host__ __device__ inline
// the body runs once, for this lane
#define PNGI_LANES(lane) for (uint32_t lane = threadIdx.x, pngi_once_ = 1; pngi_once_; pngi_once_ = 0)
#define PNGI_SYNC() __syncthreads()
#else
#define PNGI_FN inline
#define PNGI_HD inline
#define PNGI_LANES(lane) for (uint32_t lane = 0; lane < 64; lane++)
#define PNGI_SYNC() ((void)0)
#endif

namespace fpng_amd {
namespace pngi {

// statuses: the values of fpng::FPNG_DECODE_* and FPNG_AMD_DECODE_UNSUPPORTED_PNG (png_decode_api.cpp asserts it)
enum : uint32_t { kOk = 0, kNotPng = 3, kHeaderCrc = 4, kBadDims = 5, kDimsTooLarge = 6, kBadChunk = 7, kBadIdat = 8, kUnsupported = 67 };

constexpr uint32_t kWave = 64;
constexpr uint32_t kRing = 32768;    // the deflate window: the last 32 KiB of output, kept in LDS for the matches' sources
constexpr uint32_t kLitFastBits = 10, kDistFastBits = 8;
constexpr uint32_t kBandRows = 64;   // rows of the un-filter pass's skewed band: one per lane
constexpr uint32_t kTileSteps = 64;  // steps (pixels per row) that one staged tile of the band serves

// a value per lane
template <typename T> struct PngiLane {
#ifdef __HIPCC__
    T v;
    PNGI_FN T &operator[](uint32_t) { return v; }
#else
    T v[kWave];
    PNGI_FN T &operator[](uint32_t lane) { return v[lane]; }
#endif
};

// dst[lane] = src[lane - 1]; lane 0 gets `first`.  A wave operation: called outside PNGI_LANES.  dst may be src.
PNGI_FN void pngi_shift_up(PngiLane<uint32_t> &dst, PngiLane<uint32_t> &src, uint32_t first)
{
#ifdef __HIPCC__
    const uint32_t up = __shfl_up(src.v, 1);
    dst.v = threadIdx.x ? up : first;
#else
    for (uint32_t l = kWave - 1; l; l--) dst.v[l] = src.v[l - 1];
    dst.v[0] = first;
#endif
}

struct File {             // one file of a launch
    const uint8_t *data;  // the whole .png
    uint8_t *scan;        // scratch: scan_bytes, the filtered scanlines that are kept
    uint8_t *out;         // w * h * dst_c bytes (pngi_unfilter)
    uint64_t scan_bytes;  // rows * (1 + w * bpp): the image's h rows, or the y1 rows a box needs
    uint32_t size;
    uint32_t w, h;
    uint32_t color;       // IHDR colour type: 0, 2, 3, 4, 6
    uint32_t bpp;         // bytes per pixel in the file: 1, 3, 1, 2, 4
    uint32_t dst_c;       // 3 or 4
    uint64_t need_bytes;  // what the stream must yield at least, h * (1 + w * bpp); 0: scan_bytes (every row is kept)
};
struct Box {              // pngi_unfilter_box: what is stored of a file
    uint8_t *planes;      // n_planes tight planes of w x h bytes: pitch w, plane pitch w * h
    uint32_t x, y, w, h;  // inside the image, not empty
    uint32_t n_planes;    // 3 or 4 (R, G, B[, A])
    uint32_t pad_;
};
struct State {            // what pngi_inflate leaves for pngi_unfilter and the host
    uint32_t status;
    uint32_t plte_ofs, plte_n; // PLTE's data and its entries
    uint32_t trns_ofs, trns_len;
    uint32_t pad_[3];
};

// ---- the IHDR, judged on the host from the file's first 33 bytes ----
PNGI_HD uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
inline uint32_t small_crc32(const uint8_t *p, uint32_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
    }
    return ~c;
}
// head: the file's first min(size, 33) bytes.  kOk: w, h, color, bpp, file_chans are set.
inline uint32_t check_ihdr(const uint8_t *head, uint32_t size, uint32_t &w, uint32_t &h, uint32_t &color, uint32_t &bpp, uint32_t &file_chans)
{
    static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    w = h = color = bpp = file_chans = 0;
    if (size < 8 + 25 + 8 + 1 + 4 + 12) return kNotPng; // (the limit of the fpng tier's walk)
    if (memcmp(head, sig, 8) != 0 || be32(head + 8) != 13) return kNotPng;
    if (small_crc32(head + 12, 4 + 13) != be32(head + 29)) return kHeaderCrc;
    w = be32(head + 16), h = be32(head + 20);
    if (!w || !h || w > (1u << 24) || h > (1u << 24) || (uint64_t)w * h > (1u << 30)) return kBadDims;
    color = head[25];
    if (head[24] != 8 || head[26] || head[27] || head[28]) return kUnsupported; // depth, compression, filter method, interlace
    switch (color) {
    case 0: bpp = 1, file_chans = 1; break;
    case 2: bpp = 3, file_chans = 3; break;
    case 3: bpp = 1, file_chans = 3; break; // (4 with a tRNS chunk: known after the chunk walk)
    case 4: bpp = 2, file_chans = 2; break;
    case 6: bpp = 4, file_chans = 4; break;
    default: return kUnsupported;
    }
    return kOk;
}

// ---- what a wave keeps in LDS ----
struct InflateShared {
    uint16_t lit_fast[1u << kLitFastBits];   // next bits -> symbol | length << 9 (0: a longer code, or none)
    uint16_t dist_fast[1u << kDistFastBits];
    uint16_t lit_count[16], dist_count[16];  // codes per length
    uint16_t lit_sym[288], dist_sym[32];     // symbols in canonical order: the codes the fast tables do not hold
    uint16_t code[320];                      // table build: a symbol's bit-reversed code
    uint16_t next[16], offs[16];
    uint8_t lens[352];                       // (a dynamic header's lengths are read at 32 .. 348, then moved: 0 literal/length, 288 distance)
    uint32_t tok[kWave];                     // a batch of tokens: a literal's byte, or length | (distance - 1) << 9 | 1 << 31
    uint32_t tok_ofs[kWave];                 // ... and its first output byte, counted from the batch's
    uint32_t build_ok;
    uint8_t ring[kRing];
};

// ---- the bit reader: LSB first, over the data of consecutive IDAT chunks.  Every lane holds the same state. ----
struct Reader {
    const uint8_t *f;
    uint32_t size;
    uint32_t pos;    // next byte of the file
    uint32_t left;   // bytes of the current IDAT still unread
    uint64_t buf;
    uint32_t cnt;    // bits in buf
    uint32_t pad;    // of which zeros that stand in for bytes behind the last IDAT's end
    uint32_t ended;  // the IDAT chunks are used up
    uint32_t chunk_error;
    uint32_t next_chunk; // once ended: the chunk behind the last IDAT (or size)
};

// left == 0: to the next IDAT's data, over empty ones.  Ends: each round moves pos at least 12 bytes forward in a file of `size`.
PNGI_FN void pngi_next_idat(Reader &r)
{
    while (!r.left && !r.ended) {
        const uint64_t p = (uint64_t)r.pos + 4; // behind the chunk's CRC
        r.ended = 1, r.next_chunk = (uint32_t)(p < r.size ? p : r.size);
        if (p >= r.size) return;
        if (p + 12 > r.size) { r.chunk_error = 1; return; }
        const uint32_t len = be32(r.f + p);
        if (p + 12 + (uint64_t)len > r.size) { r.chunk_error = 1; return; }
        if (be32(r.f + p + 4) != 0x49444154u) return; // not IDAT: the stream's bytes end here
        r.ended = 0, r.pos = (uint32_t)p + 8, r.left = len;
    }
}

PNGI_FN void pngi_refill(Reader &r)
{
    if (r.left >= 8) { // eight bytes at once: they lie inside the chunk
        uint64_t v;
        __builtin_memcpy(&v, r.f + r.pos, 8);
        const uint32_t n = (63 - r.cnt) >> 3;
        r.buf |= v << r.cnt;
        r.pos += n, r.left -= n, r.cnt += 8 * n;
        r.buf &= (1ull << r.cnt) - 1; // (cnt <= 63)
        return;
    }
    while (r.cnt <= 56) { // ends: cnt grows by 8 a round
        if (!r.left) pngi_next_idat(r);
        uint64_t b = 0;
        if (r.left) b = r.f[r.pos++], r.left--;
        else r.pad += 8;
        r.buf |= b << r.cnt;
        r.cnt += 8;
    }
}
PNGI_FN uint32_t pngi_peek(Reader &r, uint32_t k) // k <= 32
{
    if (r.cnt < k) pngi_refill(r);
    return (uint32_t)(r.buf & ((1ull << k) - 1));
}
PNGI_FN void pngi_skip(Reader &r, uint32_t k) { r.buf >>= k, r.cnt -= k; } // (after a peek of at least k bits)
PNGI_FN uint32_t pngi_get(Reader &r, uint32_t k)
{
    const uint32_t v = pngi_peek(r, k);
    pngi_skip(r, k);
    return v;
}
// bits were taken that the file does not have
PNGI_FN bool pngi_overrun(const Reader &r) { return r.cnt < r.pad; }

// ---- Huffman tables ----
// lens[0 .. n) -> count / sym / fast (in LDS).  Lane 0 counts, checks and numbers the codes, all lanes fill the fast table.
// may_be_short: the exceptions of the literal/length and the distance code (one 1-bit code, or none; the caller refuses a
// literal/length code without the end-of-block symbol).  Returns false for an over-subscribed or incomplete code.
PNGI_FN bool pngi_build(InflateShared &sh, const uint8_t *lens, uint32_t n, uint16_t *count, uint16_t *sym, uint16_t *fast, uint32_t fast_bits, bool may_be_short)
{
    PNGI_SYNC();
    PNGI_LANES(lane)
    {
        if (lane) continue;
        for (uint32_t l = 0; l < 16; l++) count[l] = 0;
        for (uint32_t s = 0; s < n; s++) count[lens[s]]++;
        const uint32_t used = n - count[0];
        count[0] = 0;
        int32_t room = 1;
        bool ok = true;
        for (uint32_t l = 1; l < 16; l++) {
            room = room * 2 - (int32_t)count[l];
            if (room < 0) {
                ok = false;
                break;
            }
        }
        if (ok && room > 0) ok = may_be_short && (used == 0 || (used == 1 && count[1] == 1));
        sh.build_ok = ok;
        if (!ok) continue;
        uint32_t code = 0, ofs = 0;
        for (uint32_t l = 1; l < 16; l++) {
            code = (code + count[l - 1]) << 1;
            sh.next[l] = (uint16_t)code;
            sh.offs[l] = (uint16_t)ofs;
            ofs += count[l];
        }
        // sym[] in canonical order (by length, then by symbol); a symbol's code, bit-reversed
        for (uint32_t s = 0; s < n; s++) {
            const uint32_t l = lens[s];
            if (!l) continue;
            sym[sh.offs[l]++] = (uint16_t)s;
            uint32_t c = sh.next[l]++, rev = 0;
            for (uint32_t i = 0; i < l; i++, c >>= 1) rev = (rev << 1) | (c & 1);
            sh.code[s] = (uint16_t)rev;
        }
    }
    PNGI_SYNC();
    if (!sh.build_ok) return false;
    PNGI_LANES(lane)
    {
        for (uint32_t k = lane; k < (1u << fast_bits); k += kWave) fast[k] = 0;
    }
    PNGI_SYNC();
    PNGI_LANES(lane)
    {
        for (uint32_t s = lane; s < n; s += kWave) {
            const uint32_t l = lens[s];
            if (!l || l > fast_bits) continue;
            for (uint32_t k = sh.code[s]; k < (1u << fast_bits); k += 1u << l) fast[k] = (uint16_t)(s | (l << 9));
        }
    }
    PNGI_SYNC();
    return true;
}

// the next symbol, or 0xFFFF: no code of the table matches the next bits
PNGI_FN uint32_t pngi_symbol(Reader &r, const uint16_t *count, const uint16_t *sym, const uint16_t *fast, uint32_t fast_bits)
{
    const uint32_t bits = pngi_peek(r, 15);
    const uint32_t e = fast[bits & ((1u << fast_bits) - 1)];
    if (e) {
        pngi_skip(r, e >> 9);
        return e & 511;
    }
    uint32_t code = 0, first = 0, index = 0; // the canonical walk, a bit a step (15 steps at most)
    for (uint32_t l = 1; l < 16; l++) {
        code |= (bits >> (l - 1)) & 1;
        const uint32_t c = count[l];
        if (code < first + c) {
            pngi_skip(r, l);
            return sym[index + (code - first)];
        }
        index += c, first = (first + c) << 1, code <<= 1;
    }
    return 0xFFFFu;
}

// an output byte: into the window, and into the scanlines while it belongs to the image
PNGI_FN void pngi_put(InflateShared &sh, const File &f, uint64_t pos, uint32_t b)
{
    sh.ring[pos & (kRing - 1)] = (uint8_t)b;
    if (pos < f.scan_bytes) f.scan[pos] = (uint8_t)b;
}

// the tokens of a batch, in the stream's order; out: the batch's first output byte; matches: bit i = token i is a match (every lane
// holds the word, so a run of literals is found without reading the tokens back one by one)
PNGI_FN void pngi_emit(InflateShared &sh, const File &f, uint32_t n, uint64_t out, uint64_t matches)
{
    PNGI_SYNC();
    for (uint32_t i = 0; i < n;) { // ends: i grows every round
        const uint64_t rest = matches >> i;
        if (!(rest & 1)) { // a run of literals: a lane each
            const uint32_t run = rest ? (uint32_t)__builtin_ctzll(rest) : kWave, j = i + run < n ? i + run : n;
            PNGI_LANES(lane)
            {
                if (i + lane < j) pngi_put(sh, f, out + sh.tok_ofs[i + lane], sh.tok[i + lane]);
            }
            i = j;
        } else { // a match: all lanes copy; byte k comes from the window, start + k % distance where it overlaps itself
            // Storing byte dst + k takes the ring slot of byte dst + k - 32768, which for distances of 32768 - 257 and more is the
            // source of byte k - (32768 - distance) of this very match: an earlier byte, or (distance 32768) the same one.  So a
            // round of 64 bytes reads all its sources, then stores, with a barrier in between: no order among lanes is assumed,
            // and a later round's sources lie behind everything the rounds before it have overwritten.
            const uint32_t len = sh.tok[i] & 511, dist = ((sh.tok[i] >> 9) & 0xFFFF) + 1;
            const uint64_t dst = out + sh.tok_ofs[i];
            for (uint32_t k0 = 0; k0 < len; k0 += kWave) { // ends: k0 grows by 64 a round, len <= 258
                PngiLane<uint32_t> byte;
                PNGI_LANES(lane)
                {
                    const uint32_t k = k0 + lane;
                    byte[lane] = k < len ? sh.ring[(dst - dist + k % dist) & (kRing - 1)] : 0;
                }
                PNGI_SYNC();
                PNGI_LANES(lane)
                {
                    if (k0 + lane < len) pngi_put(sh, f, dst + k0 + lane, byte[lane]);
                }
                if (k0 + kWave < len) PNGI_SYNC();
            }
            i++;
        }
        PNGI_SYNC();
    }
}

// ---- the chunks from byte 33 to the first IDAT (serial and short; every read is held against the file's size) ----
PNGI_FN uint32_t pngi_walk_to_idat(const File &f, State &st, Reader &r)
{
    st.plte_ofs = st.plte_n = st.trns_ofs = st.trns_len = 0;
    bool have_plte = false;
    uint64_t ofs = 33;
    for (;;) { // ends: ofs grows by at least 12 a round
        if (ofs + 12 > f.size) return kBadChunk; // (no IDAT, or a chunk that leaves the file)
        const uint32_t len = be32(f.data + ofs), type = be32(f.data + ofs + 4);
        if (ofs + 12 + (uint64_t)len > f.size) return kBadChunk;
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t c = (type >> (8 * i)) & 255;
            if (!((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'))) return kBadChunk;
        }
        if (type == 0x49444154u) { // IDAT
            if (f.color == 3 && !have_plte) return kBadChunk;
            r.f = f.data, r.size = f.size, r.pos = (uint32_t)ofs + 8, r.left = len;
            r.buf = 0, r.cnt = 0, r.pad = 0, r.ended = 0, r.chunk_error = 0, r.next_chunk = f.size;
            return kOk;
        }
        if (type == 0x49454E44u) return kBadChunk; // IEND
        if (type == 0x504C5445u) {                 // PLTE
            if (f.color == 3 && (len % 3 || len > 768)) return kBadChunk;
            have_plte = true, st.plte_ofs = (uint32_t)ofs + 8, st.plte_n = len / 3;
        } else if (type == 0x74524E53u) // tRNS
            st.trns_ofs = (uint32_t)ofs + 8, st.trns_len = len;
        else if (!((type >> 24) & 32))
            return kUnsupported; // a critical chunk this tier does not know
        ofs += 12 + (uint64_t)len;
    }
}

// behind the stream: the chunks up to IEND (or the file's end) hold no further IDAT and no unknown critical chunk
PNGI_FN uint32_t pngi_walk_tail(Reader &r)
{
    pngi_skip(r, r.cnt & 63), r.cnt = 0, r.buf = 0;
    // IDAT data that the stream did not need
    while (!r.ended) { // ends: every round leaves a chunk of the file behind
        r.pos += r.left, r.left = 0;
        pngi_next_idat(r);
    }
    if (r.chunk_error) return kBadChunk;
    uint64_t ofs = r.next_chunk;
    while (ofs < r.size) { // ends: ofs grows by at least 12 a round
        if (ofs + 12 > r.size) return kBadChunk;
        const uint32_t len = be32(r.f + ofs), type = be32(r.f + ofs + 4);
        if (ofs + 12 + (uint64_t)len > r.size) return kBadChunk;
        if (type == 0x49444154u) return kBadChunk; // IDAT chunks that are not consecutive
        if (type == 0x49454E44u) break;
        if (type != 0x504C5445u && type != 0x74524E53u && !((type >> 24) & 32)) return kUnsupported;
        ofs += 12 + (uint64_t)len;
    }
    return kOk;
}

// ---- the stream ----
PNGI_FN uint32_t pngi_stream(InflateShared &sh, const File &f, Reader &r)
{
    const uint32_t cmf = pngi_get(r, 8), flg = pngi_get(r, 8);
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || (flg & 32) || ((cmf << 8) | flg) % 31) return kBadIdat;
    uint64_t out = 0;
    uint32_t final_block;
    do { // a block.  Ends: every block takes at least 3 bits of a bounded input (an overrun ends the walk)
        final_block = pngi_get(r, 1);
        const uint32_t type = pngi_get(r, 2);
        if (pngi_overrun(r)) return kBadIdat;
        if (type == 3) return kBadIdat;
        if (type == 0) {
            pngi_skip(r, r.cnt & 7);
            const uint32_t len = pngi_get(r, 16), nlen = pngi_get(r, 16);
            if (pngi_overrun(r) || len != (~nlen & 0xFFFF)) return kBadIdat;
            uint32_t todo = len;
            while (todo) { // ends: every round stores at least one byte of `todo` or returns
                if (r.cnt >= 8) { // the bytes the reader already holds: a lane each
                    const uint32_t n = r.cnt / 8 < todo ? r.cnt / 8 : todo;
                    if (r.cnt - 8 * n < r.pad) return kBadIdat;
                    PNGI_SYNC();
                    PNGI_LANES(lane)
                    {
                        if (lane < n) pngi_put(sh, f, out + lane, (uint32_t)(r.buf >> (8 * lane)) & 255);
                    }
                    PNGI_SYNC();
                    r.buf = n < 8 ? r.buf >> (8 * n) : 0, r.cnt -= 8 * n;
                    out += n, todo -= n;
                    continue;
                }
                if (!r.left) pngi_next_idat(r);
                if (!r.left) return kBadIdat;
                const uint32_t n = r.left < todo ? r.left : todo; // straight from the chunk
                PNGI_SYNC();
                PNGI_LANES(lane)
                {
                    for (uint32_t k = lane; k < n; k += kWave) pngi_put(sh, f, out + k, r.f[r.pos + k]);
                }
                PNGI_SYNC();
                r.pos += n, r.left -= n, out += n, todo -= n;
            }
            continue;
        }
        uint32_t n_lit = 288, n_dist = 32;
        PNGI_SYNC();
        if (type == 1) {
            PNGI_LANES(lane)
            {
                for (uint32_t s = lane; s < 320; s += kWave) sh.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
            }
        } else {
            n_lit = pngi_get(r, 5) + 257, n_dist = pngi_get(r, 5) + 1;
            const uint32_t n_clc = pngi_get(r, 4) + 4;
            if (n_lit > 286 || n_dist > 30) return kBadIdat;
            PNGI_LANES(lane)
            {
                if (lane < 19) sh.lens[lane] = 0;
            }
            PNGI_SYNC();
            for (uint32_t i = 0; i < n_clc; i++) // (every lane stores the same value)
                sh.lens[(uint8_t) "\20\21\22\0\10\7\11\6\12\5\13\4\14\3\15\2\16\1\17"[i]] = (uint8_t)pngi_get(r, 3);
            if (pngi_overrun(r)) return kBadIdat;
            // the code length code: its tables live where the distance code's will
            if (!pngi_build(sh, sh.lens, 19, sh.dist_count, sh.dist_sym, sh.dist_fast, 7, false)) return kBadIdat;
            const uint32_t total = n_lit + n_dist;
            uint32_t prev = 0;
            for (uint32_t cur = 0; cur < total;) { // ends: cur grows every round
                const uint32_t s = pngi_symbol(r, sh.dist_count, sh.dist_sym, sh.dist_fast, 7);
                if (s > 18 || pngi_overrun(r)) return kBadIdat;
                if (s < 16) {
                    sh.lens[32 + cur++] = (uint8_t)(prev = s);
                    continue;
                }
                uint32_t rep, val = 0;
                if (s == 16) {
                    if (!cur) return kBadIdat; // a repeat with nothing in front of it
                    rep = pngi_get(r, 2) + 3, val = prev;
                } else if (s == 17)
                    rep = pngi_get(r, 3) + 3, prev = 0;
                else
                    rep = pngi_get(r, 7) + 11, prev = 0;
                if (cur + rep > total) return kBadIdat;
                while (rep--) sh.lens[32 + cur++] = (uint8_t)val; // (lens[0 .. 32) are the code length code's own: still being read)
            }
            if (pngi_overrun(r)) return kBadIdat;
            PNGI_SYNC();
            if (!sh.lens[32 + 256]) return kBadIdat; // no end-of-block code
            // to their places: literal/length lengths at 0, distance lengths at 288
            PNGI_LANES(lane)
            {
                uint8_t keep[5];
                for (uint32_t k = 0; k < 5; k++) keep[k] = lane + kWave * k < total ? sh.lens[32 + lane + kWave * k] : 0;
                for (uint32_t k = 0; k < 5; k++) sh.code[lane + kWave * k] = keep[k];
            }
            PNGI_SYNC();
            PNGI_LANES(lane)
            {
                for (uint32_t s = lane; s < 320; s += kWave) sh.lens[s] = s < 288 ? (s < n_lit ? (uint8_t)sh.code[s] : 0) : (s - 288 < n_dist ? (uint8_t)sh.code[n_lit + s - 288] : 0);
            }
        }
        PNGI_SYNC();
        // (a code of one 1-bit code passes here as it does for distances: with the check above it is the end-of-block symbol alone)
        if (!pngi_build(sh, sh.lens, n_lit, sh.lit_count, sh.lit_sym, sh.lit_fast, kLitFastBits, true)) return kBadIdat;
        if (!pngi_build(sh, sh.lens + 288, n_dist, sh.dist_count, sh.dist_sym, sh.dist_fast, kDistFastBits, true)) return kBadIdat;
        for (bool eob = false; !eob;) { // a batch of up to 64 tokens.  Ends: every token takes at least one bit of a bounded input
            uint32_t n = 0, bytes = 0, bad = 0;
            uint64_t matches = 0;
            PNGI_SYNC();
            while (n < kWave) {
                const uint32_t s = pngi_symbol(r, sh.lit_count, sh.lit_sym, sh.lit_fast, kLitFastBits);
                if (s < 256) {
                    sh.tok[n] = s, sh.tok_ofs[n] = bytes; // (every lane stores the same value)
                    n++, bytes++;
                    continue;
                }
                if (s == 256) {
                    eob = true;
                    break;
                }
                if (s > 285) { // 286, 287, or no code
                    bad = 1;
                    break;
                }
                const uint32_t c = s - 257, le = c < 8 || c == 28 ? 0 : (c >> 2) - 1;
                const uint32_t len = (c < 8 ? 3 + c : c == 28 ? 258 : 3 + ((4 + (c & 3)) << le)) + pngi_get(r, le);
                const uint32_t d = pngi_symbol(r, sh.dist_count, sh.dist_sym, sh.dist_fast, kDistFastBits);
                if (d > 29) { // 30, 31, or no code
                    bad = 1;
                    break;
                }
                const uint32_t de = d < 4 ? 0 : (d >> 1) - 1;
                const uint32_t dist = (d < 4 ? 1 + d : 1 + ((2 + (d & 1)) << de)) + pngi_get(r, de);
                if (dist > out + bytes) { // in front of the first output byte
                    bad = 1;
                    break;
                }
                sh.tok[n] = len | ((dist - 1) << 9) | (1u << 31), sh.tok_ofs[n] = bytes;
                matches |= 1ull << n;
                n++, bytes += len;
            }
            if (pngi_overrun(r)) return kBadIdat; // (what was decoded from bits the file does not have is not stored)
            pngi_emit(sh, f, n, out, matches);
            out += bytes;
            if (bad) return kBadIdat;
        }
    } while (!final_block);
    if (pngi_overrun(r)) return kBadIdat;
    if (out < (f.need_bytes ? f.need_bytes : f.scan_bytes)) return kBadIdat;
    return kOk;
}

// One file: chunks, stream, chunks.  Every lane returns the same status; st is the caller's own copy.
PNGI_FN uint32_t pngi_inflate(InflateShared &sh, const File &f, State &st)
{
    Reader r;
    uint32_t status = pngi_walk_to_idat(f, st, r);
    if (!status) {
        status = pngi_stream(sh, f, r);
        if (!status && r.chunk_error) status = kBadChunk;
        // (a stream that fails where its IDAT chunks end: a chunk fault behind them -- a later IDAT, a chunk that leaves the file -- is the finding)
        const uint32_t tail = status == kOk || status == kBadIdat ? pngi_walk_tail(r) : (uint32_t)kOk;
        if (tail == kBadChunk || !status) status = tail ? tail : status;
    }
    st.status = status;
    return status;
}

// ---- un-filter and expand ----
struct UnfilterShared {
    uint32_t pal[256];   // R | G << 8 | B << 16 | A << 24
    uint8_t tile[kBandRows * (kTileSteps * 4 + 4)]; // row r: the filtered bytes of its pixels [t0 - r, t0 - r + kTileSteps); rows 4 bytes apart from a multiple of the banks
    uint8_t above[kTileSteps * 4]; // the row above the band, pixels [t0, t0 + kTileSteps), reconstructed
    uint32_t bad;
};

PNGI_FN uint32_t pngi_paeth(uint32_t a, uint32_t b, uint32_t c)
{
    const int32_t p = (int32_t)(a + b) - (int32_t)c;
    const int32_t pa = p > (int32_t)a ? p - (int32_t)a : (int32_t)a - p, pb = p > (int32_t)b ? p - (int32_t)b : (int32_t)b - p,
                  pc = p > (int32_t)c ? p - (int32_t)c : (int32_t)c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

// the store step: pixel `index` of the destination gets R, G, B[, A] of rgba
PNGI_FN void pngi_store_pixel(uint8_t *out, uint64_t index, uint32_t dst_c, uint32_t rgba)
{
    uint8_t *p = out + index * dst_c;
    p[0] = (uint8_t)rgba, p[1] = (uint8_t)(rgba >> 8), p[2] = (uint8_t)(rgba >> 16);
    if (dst_c == 4) p[3] = (uint8_t)(rgba >> 24);
}

// the box's store step: the pixel at p of the first plane gets R, G, B[, A] of rgba, a byte per plane (plane: box.w * box.h, at
// most 2^30 -- check_ihdr)
PNGI_FN void pngi_store_box(uint8_t *p, uint32_t plane, uint32_t n_planes, uint32_t rgba)
{
    p[0] = (uint8_t)rgba, p[plane] = (uint8_t)(rgba >> 8), p[2 * (uint64_t)plane] = (uint8_t)(rgba >> 16);
    if (n_planes == 4) p[3 * (uint64_t)plane] = (uint8_t)(rgba >> 24);
}

// Bands of 64 rows: lane k works on row y0 + k and, at step t, on its pixel t - k.  Its left neighbour is its own last value, the
// pixel above is the last value of lane k - 1 and the one above to the left that lane's value a step earlier: pngi_shift_up hands
// them down, no reconstructed byte goes through memory inside a band.  The band's last row is written back over its filtered
// bytes in the scanlines (all of them staged by then), where the next band's lane 0 finds it.
// The ONE walk of both entries.  kBox = false: the whole image, w x h, into f.out (box is not read).  kBox = true: rows 0 .. h - 1
// and pixels 0 .. w - 1 with w = box.x + box.w and h = box.y + box.h -- bands, tiles, staging and the write-back of lane 63's row
// end there -- and the pixels inside the box into its planes.  The scanlines' stride is the file's in both.
// (The box's place is read once per band, into what each lane keeps of its row -- where the row starts in the first plane and its
//  first pixel inside the box, none for a row above the box -- so the kernel, which hands `box` in as the record in device memory,
//  holds none of it in scalar registers across the steps: that is what keeps it free of spills.  A row's bytes, x1 * bpp and
//  w * bpp + 1 <= 2^26 + 1, are 32-bit products in the box entry for the same reason.)
template <bool kBox> PNGI_FN uint32_t pngi_unfilter_walk(UnfilterShared &sh, const File &f, const State &st, const Box &box)
{
    const uint32_t bpp = f.bpp, w = kBox ? box.x + box.w : f.w, h = kBox ? box.y + box.h : f.h, row_bytes = kTileSteps * bpp, pitch = row_bytes + 4;
    const uint64_t stride = kBox ? (uint64_t)(f.w * bpp + 1u) : (uint64_t)f.w * bpp + 1, row_end = kBox ? (uint64_t)(w * bpp) : stride - 1; // (row_end: the bytes of a row that are visited)
    const uint32_t plane = kBox ? box.w * box.h : 0u, n_planes = kBox ? box.n_planes : 0u;
    // palette, colour key
    // (the key's samples are 16-bit numbers; of an 8-bit file Pillow compares their low bytes, and so does this)
    uint32_t key = 0; // (alpha 0: no opaque pixel equals it)
    if (f.color == 0 && st.trns_len >= 2) key = f.data[st.trns_ofs + 1] | 0xFF000000u;
    else if (f.color == 2 && st.trns_len >= 6) {
        const uint8_t *t = f.data + st.trns_ofs;
        key = t[1] | (t[3] << 8) | (t[5] << 16) | 0xFF000000u;
    }
    PNGI_LANES(lane)
    {
        if (!lane) sh.bad = 0;
        if (f.color == 3)
            for (uint32_t i = lane; i < 256; i += kWave) {
                uint32_t v = 0;
                if (i < st.plte_n) {
                    const uint8_t *p = f.data + st.plte_ofs + 3 * i;
                    v = p[0] | (p[1] << 8) | (p[2] << 16) | ((i < st.trns_len ? f.data[st.trns_ofs + i] : 255u) << 24);
                }
                sh.pal[i] = v;
            }
    }
    PngiLane<uint32_t> last, up, ft, bad, x_min; // (x_min: the row's first pixel inside the box, UINT32_MAX: none)
    PngiLane<uint8_t *> box_row;                 // (... and where that pixel lies in the first plane)
    PNGI_LANES(lane) bad[lane] = 0;
    for (uint32_t y0 = 0; y0 < h; y0 += kBandRows) { // ends: h / 64 bands
        PNGI_SYNC(); // (the band above has stored its last row)
        PNGI_LANES(lane)
        {
            const uint32_t y = y0 + lane;
            uint32_t t = y < h ? f.scan[y * stride] : 0;
            if (t > 4) bad[lane] = 1, t = 0;
            ft[lane] = t, last[lane] = 0, up[lane] = 0;
            if (kBox) {
                const bool in = y >= box.y && y < h;
                x_min[lane] = in ? box.x : UINT32_MAX;
                box_row[lane] = in ? box.planes + (uint64_t)(y - box.y) * box.w : nullptr;
            }
        }
        const uint32_t rows = h - y0 < kBandRows ? h - y0 : kBandRows, steps = w + rows - 1;
        for (uint32_t t0 = 0; t0 < steps; t0 += kTileSteps) { // ends: (w + 63) / 64 tiles
            PNGI_SYNC();
            for (uint32_t r = 0; r < rows; r++) { // stage: a row's stretch is contiguous in memory
                const uint8_t *row = f.scan + (y0 + r) * stride + 1;
                PNGI_LANES(lane)
                {
                    for (uint32_t i = lane; i < row_bytes; i += kWave) {
                        const int64_t at = ((int64_t)t0 - r) * bpp + i; // byte of the row
                        sh.tile[r * pitch + i] = at >= 0 && at < (int64_t)row_end ? row[at] : 0;
                    }
                }
            }
            PNGI_LANES(lane)
            {
                for (uint32_t i = lane; i < row_bytes; i += kWave) {
                    const uint64_t at = (uint64_t)t0 * bpp + i;
                    sh.above[i] = y0 && at < row_end ? f.scan[(y0 - 1) * stride + 1 + at] : 0;
                }
            }
            PNGI_SYNC();
            const uint32_t s_end = steps - t0 < kTileSteps ? steps - t0 : kTileSteps;
            for (uint32_t s = 0; s < s_end; s++) {
                uint32_t first = 0;
                for (uint32_t c = 0; c < bpp; c++) first |= (uint32_t)sh.above[s * bpp + c] << (8 * c);
                PngiLane<uint32_t> up_left = up;
                pngi_shift_up(up, last, first);
                PNGI_LANES(lane)
                {
                    const uint32_t t = t0 + s, y = y0 + lane;
                    if (t < lane || t - lane >= w || y >= h) {
                        last[lane] = 0;
                        continue;
                    }
                    const uint32_t x = t - lane, a4 = last[lane], b4 = up[lane], c4 = up_left[lane], type = ft[lane];
                    uint32_t cur = 0;
                    for (uint32_t c = 0; c < bpp; c++) {
                        const uint32_t raw = sh.tile[lane * pitch + s * bpp + c], a = (a4 >> (8 * c)) & 255, b = (b4 >> (8 * c)) & 255, cc = (c4 >> (8 * c)) & 255;
                        const uint32_t pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : pngi_paeth(a, b, cc);
                        cur |= ((raw + pred) & 255) << (8 * c);
                    }
                    last[lane] = cur;
                    if (lane == kBandRows - 1 && y + 1 < h) // the next band's row above
                        for (uint32_t c = 0; c < bpp; c++) f.scan[y * stride + 1 + (uint64_t)x * bpp + c] = (uint8_t)(cur >> (8 * c));
                    uint32_t rgba;
                    if (f.color == 6) rgba = cur;
                    else if (f.color == 2) rgba = (cur | 0xFF000000u) == key ? cur : cur | 0xFF000000u;
                    else if (f.color == 0) rgba = (cur & 255) * 0x010101u | ((cur | 0xFF000000u) == key ? 0 : 0xFF000000u);
                    else if (f.color == 4) rgba = (cur & 255) * 0x010101u | ((cur >> 8) << 24);
                    else {
                        rgba = sh.pal[cur & 255];
                        // (the box entry: a palette index outside the box fails no file)
                        if ((cur & 255) >= st.plte_n && (!kBox || x >= x_min[lane])) bad[lane] = 1;
                    }
                    if (!kBox) pngi_store_pixel(f.out, (uint64_t)y * w + x, f.dst_c, rgba);
                    else if (x >= x_min[lane]) pngi_store_box(box_row[lane] + (x - x_min[lane]), plane, n_planes, rgba);
                }
            }
        }
    }
    PNGI_SYNC();
    PNGI_LANES(lane)
    {
        if (bad[lane]) sh.bad = 1; // (every lane that stores, stores the same value)
    }
    PNGI_SYNC();
    return sh.bad ? (uint32_t)kBadIdat : (uint32_t)kOk;
}

// the whole image, interleaved: w * h * dst_c bytes at f.out
PNGI_FN uint32_t pngi_unfilter(UnfilterShared &sh, const File &f, const State &st)
{
    const Box none = {};
    return pngi_unfilter_walk<false>(sh, f, st, none);
}

// a box of the image as planes (the rules: this file's header).  f.scan holds rows 0 .. box.y + box.h - 1 and no more
PNGI_FN uint32_t pngi_unfilter_box(UnfilterShared &sh, const File &f, const State &st, const Box &box)
{
    return pngi_unfilter_walk<true>(sh, f, st, box);
}

} // namespace pngi
} // namespace fpng_amd
