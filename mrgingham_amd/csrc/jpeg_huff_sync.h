// The Huffman decode of a baseline JPEG WITHOUT restart markers, cut into subsequences of S raw bytes that decode side by
// side and synchronise themselves: ONE text for the host (jpeg.cpp restates the whole schedule serially;
// tests/boundary/jpeg_sync_main.cpp runs it under the sanitizers) and for the device (jpeg_huff_sync.hip: one lane per
// subsequence).  DESIGN.md section 4.10 has the method and why it reaches the serial decoder's result.
//
// The state between two symbols is (p, m, k): p the next unread bit as a bit offset into the raw entropy-coded segment
// (canonical: never inside a stuffed 00), m the block inside the MCU, k the zigzag index (0: the DC symbol is next).
// jpeg_sync_lane<false> is the step F: it decodes from an entry state until p has left the subsequence -- a symbol
// belongs to the subsequence that holds its first bit -- and returns the exit state, the blocks it completed and the
// sum of the DC differences of every component.  jpeg_sync_lane<true> is the write pass: the same walk from the true
// entry, with the index of its first block and the predictors in hand, storing the non-zero luma coefficients into an
// area the caller has zeroed (a block can straddle two lanes: every coefficient has one writer) until the frame's last
// block is complete.  As in jpeg_huff_lane.h every trip of the loop decodes exactly one Huffman symbol and consumes at
// least one real bit or fails, every index that comes from the stream is checked before use, and the stream is read as
// the aligned dwords that overlap [0, len) (padded on the device, byte-exact on the host).
#pragma once
#include "jpeg_huff_lane.h"

namespace mrg {

// One subsequence's record (32 bytes, two 16-byte halves).
struct JpegSyncRecord {
    uint64_t exit;    // the state the decode left the subsequence in (jpeg_sync_pack), or kJpegSyncFailed
    uint64_t entry;   // the state it was computed from: an update round recomputes only where this differs
    uint32_t blocks;  // bits 0..15: blocks completed.  Not compared between rounds: bit 31: the decode from `entry` failed
                      // and exit/counts are the speculative ones; bits 16..30: blocks it had completed when it failed
    int32_t dc[3];    // per component, the sum of the DC differences decoded
};
static_assert(sizeof(JpegSyncRecord) == 32, "JpegSyncRecord is moved as two 16-byte halves");

// Where a subsequence begins once the file has converged (the exclusive scan over the records in front of it).
struct JpegSyncStart {
    uint32_t first_block;  // index of the block its entry lies in, in decode order; >= the frame's total: nothing to write
    int32_t pred[3];       // the DC predictors at its entry
};

constexpr uint64_t kJpegSyncFailed = (uint64_t)1 << 42;
constexpr uint32_t kJpegSyncFallback = 1u << 31;
constexpr uint32_t kJpegSyncMaxStream = 1u << 29;  // bytes: p is a 32-bit bit offset

MRG_JPEG_HD inline uint64_t jpeg_sync_pack(uint32_t bit, int m, int k) {
    return (uint64_t)bit | ((uint64_t)(uint32_t)m << 32) | ((uint64_t)(uint32_t)k << 36);
}

// what a record says that the next round compares
MRG_JPEG_HD inline bool jpeg_sync_same(const JpegSyncRecord& a, const JpegSyncRecord& b) {
    return a.exit == b.exit && ((a.blocks ^ b.blocks) & 0xFFFFu) == 0 && a.dc[0] == b.dc[0] && a.dc[1] == b.dc[1] && a.dc[2] == b.dc[2];
}

// The speculative entry of subsequence i > 0: its first byte, or the one behind it where that byte is a stuffed 00.
MRG_JPEG_HD inline uint64_t jpeg_sync_spec_entry(const uint8_t* stream, uint32_t len, uint32_t begin) {
    const uint32_t prev = (jpeg_lane_word(stream, (begin - 1) >> 2, 0, len) >> (8 * ((begin - 1) & 3))) & 0xFFu;
    return jpeg_sync_pack((begin + (prev == 0xFFu ? 1u : 0u)) * 8u, 0, 0);
}

// stream[0 .. len): the entropy-coded bytes of the file's one scan up to (not including) the first marker, so that every
// FF inside is followed by its stuffed 00; len < kJpegSyncMaxStream.  sub_end: where the subsequence ends (<= len).
// entry: jpeg_sync_pack'ed, not failed.  kWrite: `start` is the subsequence's scan result, total the blocks of the frame
// (all components), coef the frame's zeroed luma coefficients, int16 [blocks_h][pitch_blocks][64].
// Returns 0: left the subsequence (out->exit and the counts hold); 2: failed -- a code the table does not have, a DC
// category above 11, an AC size above 10, a run past coefficient 63, a bit consumed beyond len, an entry that no decode
// of this frame gives and, in the write pass, a predictor outside int16 or a block outside the area (out->blocks: the
// blocks completed until then); 1, write pass only: the frame's last block is complete.
// An entry at or behind sub_end is returned unchanged with zero counts.
template <bool kWrite>
MRG_JPEG_HD inline int jpeg_sync_lane(const uint8_t* stream, uint32_t len, uint32_t sub_end, uint64_t entry,
                                      const JpegHuffTable* tables, const uint8_t* natural, const JpegLaneGeom& g,
                                      const JpegSyncStart& start, uint32_t total, int16_t* coef, JpegSyncRecord* out) {
    out->exit = entry;
    out->entry = entry;
    out->blocks = 0;
    out->dc[0] = out->dc[1] = out->dc[2] = 0;
    const uint32_t p0 = (uint32_t)entry;
    if ((p0 >> 3) >= sub_end) return 0;
    int m = (int)((entry >> 32) & 15u), k = (int)((entry >> 36) & 63u);
    const int n0 = (int)(g.nblk & 0xFFu), n1 = (int)((g.nblk >> 8) & 0xFFu), n2 = (int)((g.nblk >> 16) & 0xFFu);
    const int bpm = n0 + n1 + n2;
    if (m >= bpm) return 2;

    // the bit reader of jpeg_huff_lane.h, entered at any bit; ffm: bit j set = the j-th last byte taken was an FF, whose
    // stuffed 00 lies between it and pos
    uint64_t acc = 0;
    int n = 0;   // valid bits at the bottom of acc
    int pad = 0;  // of which fed zeros: always the lowest ones
    uint32_t pos = p0 >> 3;  // the next unread byte
    bool after_ff = false;   // the byte at pos is the 00 stuffed behind an FF
    uint32_t ffm = 0;
    int drop = (int)(p0 & 7u);  // bits of the first byte that lie in front of the entry

    int dc0 = 0, dc1 = 0, dc2 = 0;  // F: sums of differences; write pass: the predictors
    uint32_t blocks = 0, blk = 0, mx = 0, my = 0;
    int16_t* dst = nullptr;  // the luma block being filled
    if (kWrite) {
        dc0 = start.pred[0];
        dc1 = start.pred[1];
        dc2 = start.pred[2];
        blk = start.first_block;
        if (blk >= total || blk % (uint32_t)bpm != (uint32_t)m) return 2;
        const uint32_t mcu = blk / (uint32_t)bpm;
        mx = mcu % (uint32_t)g.mcus_x;
        my = mcu / (uint32_t)g.mcus_x;
        if (m < n0 && k > 0) {  // entered inside a luma block
            const uint32_t bx = mx * (uint32_t)g.H0 + (uint32_t)(m % g.H0), by = my * (uint32_t)g.V0 + (uint32_t)(m / g.H0);
            if (bx >= (uint32_t)g.pitch_blocks || by >= (uint32_t)g.blocks_h) return 2;
            dst = coef + ((size_t)by * (size_t)g.pitch_blocks + bx) * 64;
        }
    }

    for (;;) {
        if (n < 32) {  // a code (<= 16 bits) and its value bits (<= 11) fit
            if (pos < len) {
                const uint32_t w = jpeg_lane_word(stream, pos >> 2, 0, len);
                const uint32_t base = pos & ~3u;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t p = base + j;
                    if (p < pos || p >= len) continue;
                    const uint32_t b = (w >> (8 * j)) & 0xFFu;
                    if (!after_ff) {
                        acc = (acc << 8) | b;
                        n += 8;
                        ffm = (ffm << 1) | (b == 0xFFu ? 1u : 0u);
                    }
                    after_ff = !after_ff && b == 0xFFu;
                }
                pos = base + 4 < len ? base + 4 : len;
                continue;  // (n < 32 again: one more dword; at most 32 bits are added to fewer than 32)
            }
            acc <<= 32;
            n += 32;
            pad += 32;
        }
        if (drop) {  // (the entry's byte is real: pos < sub_end <= len)
            n -= drop;
            drop = 0;
            continue;
        }
        const int c = m < n0 ? 0 : m < n0 + n1 ? 1 : 2;
        const uint32_t slot = (g.slots >> (4 * (k == 0 ? c : 4 + c))) & 15u;
        const JpegHuffTable& t = tables[slot < (uint32_t)kJpegLaneTables ? slot : 0];
        // one symbol
        int sym, slen;
        const uint32_t e = t.look[(uint32_t)(acc >> (n - kJpegLookBits)) & ((1u << kJpegLookBits) - 1u)];
        if (e) {
            slen = (int)(e >> 8);
            sym = (int)(e & 0xFFu);
        } else {
            sym = -1;
            slen = 0;
            for (int l = kJpegLookBits + 1; l <= 16; ++l) {
                const int32_t code = (int32_t)((uint32_t)(acc >> (n - l)) & ((1u << l) - 1u));
                if (code <= t.maxcode[l]) {
                    const int idx = code + t.valoff[l];
                    if (idx >= 0 && idx < t.nvals && idx < 256) {
                        sym = t.vals[idx];
                        slen = l;
                    }
                    break;
                }
            }
            if (sym < 0) break;
        }
        n -= slen;
        const int s = k == 0 ? sym : sym & 15;
        int v = 0;
        if (s) {
            if (s > (k == 0 ? 11 : 10)) break;
            v = (int)((uint32_t)(acc >> (n - s)) & ((1u << s) - 1u));
            n -= s;
            if (v < (1 << (s - 1))) v += 1 - (1 << s);
        }
        if (n < pad) break;  // a bit beyond `len` was consumed
        bool block_done = false;
        if (k == 0) {  // the DC difference: summed (F), or put onto the component's predictor (write pass)
            const int pred = (c == 0 ? dc0 : c == 1 ? dc1 : dc2) + v;
            if (kWrite && (pred < -32768 || pred > 32767)) break;
            if (c == 0) dc0 = pred;
            else if (c == 1) dc1 = pred;
            else dc2 = pred;
            if (kWrite) {
                dst = nullptr;
                if (c == 0) {
                    const uint32_t bx = mx * (uint32_t)g.H0 + (uint32_t)(m % g.H0), by = my * (uint32_t)g.V0 + (uint32_t)(m / g.H0);
                    if (bx >= (uint32_t)g.pitch_blocks || by >= (uint32_t)g.blocks_h) break;
                    dst = coef + ((size_t)by * (size_t)g.pitch_blocks + bx) * 64;
                    if (pred) dst[0] = (int16_t)pred;
                }
            }
            k = 1;
        } else {
            const int r = sym >> 4;
            if (s == 0) {
                if (r != 15) {
                    block_done = true;  // end of block (r != 0: a progressive file's EOB run has no meaning here)
                } else {
                    if (k + 15 > 63) break;  // sixteen zeros that do not fit
                    k += 16;
                }
            } else {
                k += r;
                if (k > 63) break;
                if (kWrite && dst && v) dst[natural[k]] = (int16_t)v;
                ++k;
            }
            if (k > 63) block_done = true;
        }
        if (block_done) {
            k = 0;
            ++blocks;
            if (++m >= bpm) {
                m = 0;
                if (++mx >= (uint32_t)g.mcus_x) { mx = 0; ++my; }
            }
            if (kWrite && ++blk >= total) {  // the frame is complete: what follows is not examined
                out->blocks = blocks;
                return 1;
            }
        }
        // where the next unread bit lies: u bytes of acc are unread or partly read; behind each FF among them lies a 00
        const int r = n - pad;
        const uint32_t u = (uint32_t)(r + 7) >> 3;
        // (u == 0 with after_ff set -- every byte read and pos on the 00 behind the last one, an FF -- makes `back` wrap to
        // 2^32 - 1 and `byte` pos + 1, modulo 2^32: the bit behind the stuffed 00, as it has to be)
        const uint32_t back = u + (uint32_t)__builtin_popcount(ffm & ((1u << u) - 1u)) - (after_ff ? 1u : 0u);
        const uint32_t byte = pos - back;
        if (byte >= sub_end) {
            out->exit = jpeg_sync_pack(byte * 8u + ((8u - ((uint32_t)r & 7u)) & 7u), m, k);
            out->blocks = blocks;
            out->dc[0] = dc0;
            out->dc[1] = dc1;
            out->dc[2] = dc2;
            return 0;
        }
    }
    out->blocks = blocks;
    return 2;
}

// Round 0: the record of a subsequence decoded from `entry` (the file's true start for the first one, the speculative
// entry for the others).
MRG_JPEG_HD inline void jpeg_sync_speculate(const uint8_t* stream, uint32_t len, uint32_t sub_end, uint64_t entry,
                                            const JpegHuffTable* tables, const uint8_t* natural, const JpegLaneGeom& g,
                                            JpegSyncRecord* out) {
    const JpegSyncStart none = {0, {0, 0, 0}};
    if (jpeg_sync_lane<false>(stream, len, sub_end, entry, tables, natural, g, none, 0, nullptr, out) != 0) {
        out->exit = kJpegSyncFailed;
        out->blocks = kJpegSyncFallback | ((out->blocks & 0x7FFFu) << 16);
        out->dc[0] = out->dc[1] = out->dc[2] = 0;
    }
    out->entry = entry;
}

// One update: the record of subsequence i from the record in front of it (`before`: its own record of the last round,
// `spec`: its record of round 0).  An unchanged entry carries the record forward; a failed entry, or a decode that
// fails, falls back to the speculative record.  Returns whether the record differs from `before` in what is compared.
MRG_JPEG_HD inline bool jpeg_sync_update(const uint8_t* stream, uint32_t len, uint32_t sub_end, const JpegSyncRecord& prev,
                                         const JpegSyncRecord& before, const JpegSyncRecord& spec, const JpegHuffTable* tables,
                                         const uint8_t* natural, const JpegLaneGeom& g, JpegSyncRecord* out) {
    const uint64_t entry = prev.exit;
    if (before.entry == entry) {
        *out = before;
        return false;
    }
    int rc = 2;
    uint32_t partial = 0;
    if (!(entry & kJpegSyncFailed)) {
        const JpegSyncStart none = {0, {0, 0, 0}};
        rc = jpeg_sync_lane<false>(stream, len, sub_end, entry, tables, natural, g, none, 0, nullptr, out);
        partial = out->blocks & 0x7FFFu;
    }
    if (rc != 0) {
        *out = spec;
        out->blocks = (spec.blocks & 0xFFFFu) | kJpegSyncFallback | (partial << 16);
    }
    out->entry = entry;
    return !jpeg_sync_same(*out, before);
}

}  // namespace mrg
