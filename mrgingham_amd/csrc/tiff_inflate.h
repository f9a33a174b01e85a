// The Deflate decoder of one TIFF strip (compression 8 / 32946: a zlib stream, RFC 1950 around RFC 1951), one text for the
// differential program of the tests and the device kernel (tiff_decode.hip: one lane per strip), like tiff_lzw.h.
//
// The contract is zlib's: tiff_inflate_decode returns kTiffInflateOk exactly when uncompress() into a buffer of exactly
// `nout` bytes returns Z_OK with `nout` bytes -- the test of the host decoder (image_io.cpp: decode_tiff) -- and the bytes
// are then the same.  So, unlike the LZW text, the decoder does NOT stop when `nout` bytes are out: it goes on through
// blocks that give nothing to the final block and checks the Adler-32; bytes behind the trailer are ignored.  Of zlib's
// ways with odd streams it keeps these: a code set may be incomplete only if it is a single code of one bit (literal /
// length and distance sets; the code-length code must be complete), a block may come without any distance code, using a
// code that is not there is an error, and the window size of the header bounds nothing but itself (CINFO <= 7).
//
// Memory: never reads beyond src + nsrc, never writes beyond out + nout (an overrun is found before the store), and a
// distance larger than the bytes already out in THIS strip is an error -- the copy source is the strip's own output.
//
// The decoder keeps its decode tables and the code-length work area in kTiffInflateWords 16-bit words, 2560 bytes; where
// they live is the template parameter: anything with get(i) and set(i, v) for i < kTiffInflateWords.  A code set is held
// as a root table over the next 9 (distances: 6, code lengths: 7) bits -- symbol << 4 | length, 0 where the code is
// longer -- and, for the longer codes, the counts per length and the symbols in code order (canonical decoding, a length
// at a time).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRG_INFLATE_HD __host__ __device__ inline
// The loops over table words stay loops on the device.  Unrolled, the compiler keeps the addresses of hundreds of words in
// registers and a wave gets a SIMD to itself; the kernel lives on many waves hiding each other's memory latency.
#define MRG_INFLATE_LOOP _Pragma("unroll 1")
#define MRG_INFLATE_UNROLL _Pragma("unroll")
#else
#define MRG_INFLATE_HD inline
#define MRG_INFLATE_LOOP
#define MRG_INFLATE_UNROLL
#endif

namespace mrg {

// what tiff_inflate_decode / tiff_inflate_raw return
constexpr int kTiffInflateOk = 0;
constexpr int kTiffInflateHeader = 1;      // the two zlib header bytes: CM, CINFO, FCHECK or FDICT
constexpr int kTiffInflateCutShort = 2;    // the bytes end inside a block or inside the trailer
constexpr int kTiffInflateBlockType = 3;   // block type 3
constexpr int kTiffInflateStoredLen = 4;   // a stored block's LEN and NLEN do not match
constexpr int kTiffInflateCounts = 5;      // HLIT above 286 or HDIST above 30
constexpr int kTiffInflateCodeSet = 6;     // an over-subscribed code set, or an incomplete one that zlib does not take
constexpr int kTiffInflateRepeat = 7;      // repeat code 16 first, or a repeat running over the end of the lengths
constexpr int kTiffInflateNoEnd = 8;       // no end-of-block code
constexpr int kTiffInflateBadCode = 9;     // a code that is not in its set; literal/length symbol 286 / 287, distance symbol 30 / 31
constexpr int kTiffInflateDistance = 10;   // a distance beyond the bytes out in this strip
constexpr int kTiffInflateTooLong = 11;    // more than `nout` bytes
constexpr int kTiffInflateTooShort = 12;   // the final block ends with fewer than `nout` bytes out
constexpr int kTiffInflateChecksum = 13;   // the Adler-32 of the trailer is not that of the bytes

// What the device route takes.  Unlike an LZW code, a Deflate block need not give a byte, and every block with a code of
// its own costs its tables: the work of a lane is bounded by the strip's COMPRESSED bytes, not by what it decodes to.  So
// both are limited: a strip decodes to at most 1 MiB, and its bytes in the file are at most what it decodes to plus an
// eighth plus 512 -- no choice of zlib's gives more (the fixed code spends 9 bits on a byte at worst, stored blocks 5 bytes
// per block), and the slack has room for the longest header of a dynamic block (under 300 bytes) around a strip of a few
// bytes, for a sync flush or for bytes behind the trailer.  A strip with more bytes than that
// keeps the host decoder, which walks them in no time.
constexpr uint32_t kTiffInflateMaxStrip = 1u << 20;
MRG_INFLATE_HD unsigned long long tiff_inflate_max_bytes(unsigned long long decoded) { return decoded + decoded / 8 + 512; }

// the layout of the table words
constexpr int kTiffInflateLitRootBits = 9, kTiffInflateDistRootBits = 6, kTiffInflateClRootBits = 7;
constexpr int kTiffInflateLens = 0;                                            // 320: the code lengths of a block, literal/length then distance
constexpr int kTiffInflateLitSym = kTiffInflateLens + 320;                     // 288 (the code-length code's 19 lengths and symbols meanwhile)
constexpr int kTiffInflateDistSym = kTiffInflateLitSym + 288;                  // 32
constexpr int kTiffInflateLitCount = kTiffInflateDistSym + 32;                 // 16 counts per length, 16 offsets while sorting
constexpr int kTiffInflateDistCount = kTiffInflateLitCount + 32;               // 32
constexpr int kTiffInflateLitRoot = kTiffInflateDistCount + 32;                // 512 (the code-length code's root table while lengths are read)
constexpr int kTiffInflateDistRoot = kTiffInflateLitRoot + 512;                // 64
constexpr int kTiffInflateWords = 1280;
static_assert(kTiffInflateDistRoot + 64 == kTiffInflateWords, "the table words stated above");

// the host's arrangement: the words side by side
struct TiffInflateHostTable {
    uint16_t w[kTiffInflateWords];
    uint32_t get(int i) const { return w[i]; }
    void set(int i, uint32_t v) { w[i] = (uint16_t)v; }
};

// words `stride` apart (the kernel: the tables of the lanes of a launch interleaved by lane, so that the lanes of a wave
// touch consecutive words)
struct TiffInflateStridedTable {
    uint16_t* word;  // word i at word[i * stride]
    uint32_t stride;
    MRG_INFLATE_HD uint32_t get(int i) const { return word[(uint32_t)i * stride]; }
    MRG_INFLATE_HD void set(int i, uint32_t v) { word[(uint32_t)i * stride] = (uint16_t)v; }
};

namespace inflate_detail {

// the input: bits LSB first; `hold` has the next `bits` bits, zeros above them
struct Bits {
    const uint8_t* src;
    uint32_t nsrc, in;
    uint64_t hold;
    int bits;
    // To at least 33 bits, or to the end of the bytes: four bytes at once while there are four (one wait for memory per
    // four bytes, not per byte), the last ones singly.  Nothing between two refills takes more than 28 bits.
    MRG_INFLATE_HD void refill() {
        if (bits > 32) return;
        if (nsrc - in >= 4) {
            const uint32_t w = src[in] | (uint32_t)src[in + 1] << 8 | (uint32_t)src[in + 2] << 16 | (uint32_t)src[in + 3] << 24;
            hold |= (uint64_t)w << bits;
            in += 4;
            bits += 32;
            return;
        }
        while (bits <= 56 && in < nsrc) {
            hold |= (uint64_t)src[in++] << bits;
            bits += 8;
        }
    }
    MRG_INFLATE_HD uint32_t peek(int n) const { return (uint32_t)hold & ((1u << n) - 1u); }
    MRG_INFLATE_HD void drop(int n) { hold >>= n; bits -= n; }
    // to the next byte boundary, the whole bytes held given back: `in` is then the position of the next unused byte
    MRG_INFLATE_HD void to_byte() {
        in -= (uint32_t)(bits >> 3);
        hold = 0;
        bits = 0;
    }
};

// n bytes from `from` to `to`, where the first byte written lies at least 8 bytes behind the first byte read or in another
// block altogether: eight bytes are read before any of them is written, one wait for memory per eight bytes
MRG_INFLATE_HD void copy_apart(const uint8_t* from, uint8_t* to, uint32_t n) {
    uint32_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t v = 0;
        MRG_INFLATE_UNROLL
        for (int k = 0; k < 8; ++k) v |= (uint64_t)from[i + k] << (8 * k);
        MRG_INFLATE_UNROLL
        for (int k = 0; k < 8; ++k) to[i + k] = (uint8_t)(v >> (8 * k));
    }
    for (; i < n; ++i) to[i] = from[i];
}

MRG_INFLATE_HD uint32_t reverse_bits(uint32_t code, int len) {
    uint32_t r = 0;
    MRG_INFLATE_LOOP
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// The code set of the n lengths at words [lens, lens + n): counts at [count, count + 16) (and sorting offsets behind them),
// symbols in code order at [sym, sym + n), root table at [root, root + 2^root_bits).  zlib's rules (inflate_table): an
// over-subscribed set is refused; an incomplete one too, unless -- may_be_incomplete -- it has no code at all or one code
// of one bit.
template <class Table>
MRG_INFLATE_HD bool build(Table& t, int lens, int n, int count, int sym, int root, int root_bits, bool may_be_incomplete) {
    MRG_INFLATE_LOOP
    for (int i = 0; i < 16; ++i) t.set(count + i, 0);
    MRG_INFLATE_LOOP
    for (int i = 0; i < n; ++i) {
        const int l = (int)t.get(lens + i);
        t.set(count + l, t.get(count + l) + 1);
    }
    int left = 1, max = 0, off = 0;
    MRG_INFLATE_LOOP
    for (int l = 1; l <= 15; ++l) {
        const int c = (int)t.get(count + l);
        left = (left << 1) - c;
        if (left < 0) return false;
        if (c) max = l;
        t.set(count + 16 + l, (uint32_t)off);
        off += c;
    }
    if (left > 0 && !(may_be_incomplete && max <= 1)) return false;
    MRG_INFLATE_LOOP
    for (int i = 0; i < n; ++i) {
        const int l = (int)t.get(lens + i);
        if (l == 0) continue;
        const uint32_t at = t.get(count + 16 + l);
        t.set(sym + (int)at, (uint32_t)i);
        t.set(count + 16 + l, at + 1);
    }
    const int size = 1 << root_bits;
    MRG_INFLATE_LOOP
    for (int i = 0; i < size; ++i) t.set(root + i, 0);
    uint32_t code = 0;
    int index = 0;
    MRG_INFLATE_LOOP
    for (int l = 1; l <= root_bits; ++l) {
        const int c = (int)t.get(count + l);
        MRG_INFLATE_LOOP
        for (int k = 0; k < c; ++k, ++index, ++code) {
            const uint32_t entry = t.get(sym + index) << 4 | (uint32_t)l;
            MRG_INFLATE_LOOP
            for (uint32_t j = reverse_bits(code, l); j < (uint32_t)size; j += 1u << l) t.set(root + (int)j, entry);
        }
        code <<= 1;
    }
    return true;
}

// the next symbol of a code set, or -1 (a code that is not there) / -2 (the bits end inside it)
template <class Table>
MRG_INFLATE_HD int symbol(const Table& t, Bits& b, int count, int sym, int root, int root_bits) {
    const uint32_t next = b.peek(15);
    const uint32_t e = t.get(root + (int)(next & ((1u << root_bits) - 1u)));
    int len = (int)(e & 15u), s = (int)(e >> 4);
    if (e == 0) {
        s = -1;
        int code = 0, first = 0, index = 0;
        MRG_INFLATE_LOOP
        for (len = 1; len <= 15; ++len) {
            code |= (int)((next >> (len - 1)) & 1u);
            const int c = (int)t.get(count + len);
            if (code - c < first) {
                s = (int)t.get(sym + index + (code - first));
                break;
            }
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        if (s < 0) return -1;
    }
    if (len > b.bits) return -2;
    b.drop(len);
    return s;
}

// length symbols 257 .. 285 and distance symbols 0 .. 29: base = first value, extra bits (RFC 1951, 3.2.5)
MRG_INFLATE_HD void length_of(int s, uint32_t* base, int* extra) {
    const int i = s - 257;
    if (i < 8) { *base = 3u + (uint32_t)i; *extra = 0; }
    else if (i == 28) { *base = 258; *extra = 0; }
    else {
        const int e = (i >> 2) - 1;
        *extra = e;
        *base = 3u + ((4u + (uint32_t)(i & 3)) << e);
    }
}
MRG_INFLATE_HD void distance_of(int s, uint32_t* base, int* extra) {
    if (s < 4) { *base = 1u + (uint32_t)s; *extra = 0; }
    else {
        const int e = (s >> 1) - 1;
        *extra = e;
        *base = 1u + ((2u + (uint32_t)(s & 1)) << e);
    }
}

}  // namespace inflate_detail

// The raw Deflate stream (RFC 1951) at src[*in_at, nsrc): all its blocks, to the end of the final one.  Then *in_at is the
// position of the first byte behind the stream (the final block's last byte taken whole).  Exactly `nout` bytes, or an error.
template <class Table>
MRG_INFLATE_HD int tiff_inflate_blocks(const uint8_t* src, uint32_t nsrc, uint32_t* in_at, uint8_t* out, uint32_t nout, Table& t) {
    using namespace inflate_detail;
    constexpr int kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    Bits b{src, nsrc, *in_at, 0, 0};
    uint32_t o = 0;
    bool fixed_built = false;  // the tables hold the fixed code: the next fixed block of the strip takes them as they are
    for (bool last = false; !last;) {
        b.refill();
        if (b.bits < 3) return kTiffInflateCutShort;
        last = b.peek(1) != 0;
        const uint32_t type = b.peek(3) >> 1;
        b.drop(3);
        if (type == 3) return kTiffInflateBlockType;
        if (type == 0) {
            b.drop(b.bits & 7);
            b.to_byte();
            if (nsrc - b.in < 4) return kTiffInflateCutShort;
            const uint32_t len = src[b.in] | (uint32_t)src[b.in + 1] << 8, nlen = src[b.in + 2] | (uint32_t)src[b.in + 3] << 8;
            b.in += 4;
            if ((len ^ 0xFFFFu) != nlen) return kTiffInflateStoredLen;
            if (len > nout - o) return kTiffInflateTooLong;
            if (len > nsrc - b.in) return kTiffInflateCutShort;
            copy_apart(src + b.in, out + o, len);
            o += len;
            b.in += len;
            continue;
        }
        int nlen = 288, ndist = 32;
        const bool built = type == 1 && fixed_built;
        fixed_built = type == 1;
        if (type == 1) {  // the fixed code: 288 and 32 symbols, the last two of each never to be used
            MRG_INFLATE_LOOP
            for (int i = 0; i < 288 && !built; ++i) t.set(kTiffInflateLens + i, i < 144 ? 8u : i < 256 ? 9u : i < 280 ? 7u : 8u);
            MRG_INFLATE_LOOP
            for (int i = 0; i < 32 && !built; ++i) t.set(kTiffInflateLens + 288 + i, 5u);
        } else {
            if (b.bits < 14) return kTiffInflateCutShort;
            nlen = (int)b.peek(5) + 257;
            b.drop(5);
            ndist = (int)b.peek(5) + 1;
            b.drop(5);
            const int ncode = (int)b.peek(4) + 4;
            b.drop(4);
            if (nlen > 286 || ndist > 30) return kTiffInflateCounts;
            // the code-length code, its 19 lengths where the literal symbols will lie
            MRG_INFLATE_LOOP
            for (int i = 0; i < 19; ++i) t.set(kTiffInflateLitSym + 32 + i, 0);
            MRG_INFLATE_LOOP
            for (int i = 0; i < ncode; ++i) {
                b.refill();
                if (b.bits < 3) return kTiffInflateCutShort;
                t.set(kTiffInflateLitSym + 32 + kOrder[i], b.peek(3));
                b.drop(3);
            }
            if (!build(t, kTiffInflateLitSym + 32, 19, kTiffInflateLitCount, kTiffInflateLitSym, kTiffInflateLitRoot, kTiffInflateClRootBits, false))
                return kTiffInflateCodeSet;
            MRG_INFLATE_LOOP
            for (int have = 0; have < nlen + ndist;) {
                b.refill();
                const int s = symbol(t, b, kTiffInflateLitCount, kTiffInflateLitSym, kTiffInflateLitRoot, kTiffInflateClRootBits);
                if (s < 0) return s == -1 ? kTiffInflateBadCode : kTiffInflateCutShort;
                if (s < 16) {
                    t.set(kTiffInflateLens + have++, (uint32_t)s);
                    continue;
                }
                uint32_t value = 0;
                int extra = 2, base = 3;
                if (s == 16) {
                    if (have == 0) return kTiffInflateRepeat;
                    value = t.get(kTiffInflateLens + have - 1);
                } else if (s == 17) {
                    extra = 3;
                } else {
                    extra = 7;
                    base = 11;
                }
                if (b.bits < extra) return kTiffInflateCutShort;
                const int repeat = base + (int)b.peek(extra);
                b.drop(extra);
                if (have + repeat > nlen + ndist) return kTiffInflateRepeat;
                MRG_INFLATE_LOOP
                for (int i = 0; i < repeat; ++i) t.set(kTiffInflateLens + have++, value);
            }
            if (t.get(kTiffInflateLens + 256) == 0) return kTiffInflateNoEnd;
        }
        if (!built &&
            (!build(t, kTiffInflateLens, nlen, kTiffInflateLitCount, kTiffInflateLitSym, kTiffInflateLitRoot, kTiffInflateLitRootBits, true) ||
            !build(t, kTiffInflateLens + nlen, ndist, kTiffInflateDistCount, kTiffInflateDistSym, kTiffInflateDistRoot, kTiffInflateDistRootBits, true)))
            return kTiffInflateCodeSet;
        for (;;) {
            b.refill();
            int s = symbol(t, b, kTiffInflateLitCount, kTiffInflateLitSym, kTiffInflateLitRoot, kTiffInflateLitRootBits);
            if (s < 0) return s == -1 ? kTiffInflateBadCode : kTiffInflateCutShort;
            if (s < 256) {
                if (o >= nout) return kTiffInflateTooLong;
                out[o++] = (uint8_t)s;
                continue;
            }
            if (s == 256) break;
            if (s > 285) return kTiffInflateBadCode;
            uint32_t len, dist;
            int extra;
            length_of(s, &len, &extra);
            if (b.bits < extra) return kTiffInflateCutShort;
            len += b.peek(extra);
            b.drop(extra);
            b.refill();
            s = symbol(t, b, kTiffInflateDistCount, kTiffInflateDistSym, kTiffInflateDistRoot, kTiffInflateDistRootBits);
            if (s < 0) return s == -1 ? kTiffInflateBadCode : kTiffInflateCutShort;
            if (s > 29) return kTiffInflateBadCode;
            distance_of(s, &dist, &extra);
            if (b.bits < extra) return kTiffInflateCutShort;
            dist += b.peek(extra);
            b.drop(extra);
            if (dist > o) return kTiffInflateDistance;
            if (len > nout - o) return kTiffInflateTooLong;
            if (dist >= 8) {
                copy_apart(out + o - dist, out + o, len);
            } else {  // the copy runs into what it writes: the `dist` bytes before it, over and over
                uint64_t period = 0;
                MRG_INFLATE_LOOP
                for (uint32_t k = 0; k < dist; ++k) period |= (uint64_t)out[o - dist + k] << (8 * k);
                uint32_t k = 0;
                MRG_INFLATE_LOOP
                for (uint32_t i = 0; i < len; ++i) {
                    out[o + i] = (uint8_t)(period >> (8 * k));
                    k = k + 1 == dist ? 0 : k + 1;
                }
            }
            o += len;
        }
    }
    if (o != nout) return kTiffInflateTooShort;
    b.drop(b.bits & 7);
    b.to_byte();
    *in_at = b.in;
    return kTiffInflateOk;
}

// a raw Deflate stream of exactly `nout` bytes (zlib: inflateInit2(-15)); what follows the final block is ignored
template <class Table>
MRG_INFLATE_HD int tiff_inflate_raw(const uint8_t* src, uint32_t nsrc, uint8_t* out, uint32_t nout, Table& t) {
    uint32_t in = 0;
    return tiff_inflate_blocks(src, nsrc, &in, out, nout, t);
}

// a zlib stream of exactly `nout` bytes (zlib: uncompress); what follows the trailer is ignored
template <class Table>
MRG_INFLATE_HD int tiff_inflate_decode(const uint8_t* src, uint32_t nsrc, uint8_t* out, uint32_t nout, Table& t) {
    if (nsrc < 2) return kTiffInflateCutShort;
    const uint32_t cmf = src[0], flg = src[1];
    if ((cmf << 8 | flg) % 31u != 0 || (cmf & 15u) != 8 || (cmf >> 4) > 7 || (flg & 32u)) return kTiffInflateHeader;
    uint32_t in = 2;
    const int rc = tiff_inflate_blocks(src, nsrc, &in, out, nout, t);
    if (rc) return rc;
    if (nsrc - in < 4) return kTiffInflateCutShort;
    uint32_t a = 1, s = 0;  // Adler-32: the sums reduced every 5552 bytes, before they can pass 2^32
    for (uint32_t i = 0; i < nout;) {
        const uint32_t end = nout - i > 5552u ? i + 5552u : nout;
        for (; i < end; ++i) {
            a += out[i];
            s += a;
        }
        a %= 65521u;
        s %= 65521u;
    }
    const uint32_t want = (uint32_t)src[in] << 24 | (uint32_t)src[in + 1] << 16 | (uint32_t)src[in + 2] << 8 | src[in + 3];
    return want == (s << 16 | a) ? kTiffInflateOk : kTiffInflateChecksum;
}

}  // namespace mrg
