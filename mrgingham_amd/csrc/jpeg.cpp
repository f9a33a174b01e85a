// See jpeg.h.
#include "jpeg.h"
#include "jpeg_huff_lane.h"
#include "jpeg_idct8.h"

#include <string.h>

namespace mrg {
namespace {

constexpr int kMaxSide = 32767;  // as image_io.cpp: checked before anything is sized from a header field

const uint8_t kNatural[64] = {MRG_JPEG_NATURAL_ORDER};  // position in the zigzag scan -> position in the block

constexpr int kLookBits = kJpegLookBits;

using Huff = JpegHuffTable;  // (jpeg_huff_lane.h: the 9-bit look-up and the canonical walk, flat)

// counts[16] + symbols, as a DHT segment holds them.  false: the lengths do not describe a prefix code.
bool build_huff(Huff& h, const uint8_t* counts, const uint8_t* vals, int nvals) {
    memset(&h, 0, sizeof(h));
    memcpy(h.vals, vals, (size_t)nvals);
    h.nvals = nvals;
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = counts[l - 1];
        h.valoff[l] = k - code;
        if (n) {
            if (code + n > (1 << l)) return false;
            if (l <= kLookBits)
                for (int i = 0; i < n; ++i) {
                    const int first = (code + i) << (kLookBits - l);
                    for (int j = 0; j < 1 << (kLookBits - l); ++j) h.look[first + j] = (uint16_t)((l << 8) | vals[k + i]);
                }
            code += n;
            k += n;
            h.maxcode[l] = code - 1;
        } else {
            h.maxcode[l] = -1;
        }
        code <<= 1;
    }
    h.defined = 1;
    return true;
}

// The entropy-coded bytes of one restart interval.  Where the data ends (the end of the file, or any marker) zero bits
// are fed and counted: a decoder that has CONSUMED one of them has read past the data, which the caller reports.
struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc = 0;
    int n = 0;    // valid bits at the bottom of acc
    int pad = 0;  // of which fed zeros: always the lowest ones

    void fill() {
        while (n <= 48) {
            unsigned b = 0;
            if (pad == 0 && p < end) {
                b = *p;
                if (b != 0xFF) ++p;
                else if (p + 1 < end && p[1] == 0) p += 2;  // a stuffed FF 00
                else { b = 0; pad = 8; }                    // a marker (p stays on it), or FF as the last byte
            } else {
                pad += 8;
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    void need() { if (n < 32) fill(); }  // a code (<= 16 bits) and its value bits (<= 11) fit
    unsigned peek(int k) const { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1u); }
    unsigned take(int k) { const unsigned v = peek(k); n -= k; return v; }
    bool overrun() const { return n < pad; }
};

// one Huffman symbol, or -1: no such code
inline int decode_symbol(Bits& b, const Huff& h) {
    const unsigned e = h.look[b.peek(kLookBits)];
    if (e) { b.n -= (int)(e >> 8); return (int)(e & 0xFF); }
    for (int l = kLookBits + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)b.peek(l);
        if (code <= h.maxcode[l]) {
            const int idx = code + h.valoff[l];
            if (idx < 0 || idx >= h.nvals) return -1;
            b.n -= l;
            return h.vals[idx];
        }
    }
    return -1;
}

inline int receive_extend(Bits& b, int s) {
    const int v = (int)b.take(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block: the DC difference onto *pred, then the AC run lengths.  dst (64 coefficients, natural order) may be NULL:
// a chroma block, decoded only to get past it.
bool decode_block(Bits& b, const Huff& dc, const Huff& ac, int* pred, int16_t* dst) {
    b.need();
    int s = decode_symbol(b, dc);
    if (s < 0 || s > 11) return false;
    if (s) *pred += receive_extend(b, s);
    if (*pred < -32768 || *pred > 32767) return false;
    if (dst) {
        memset(dst, 0, 64 * sizeof(int16_t));
        dst[0] = (int16_t)*pred;
    }
    for (int k = 1; k < 64;) {
        b.need();
        const int rs = decode_symbol(b, ac);
        if (rs < 0) return false;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;            // end of block (r != 0: a progressive file's EOB run has no meaning here)
            if (k + 15 > 63) return false;  // sixteen zeros that do not fit
            k += 16;
            continue;
        }
        k += r;
        if (k > 63 || s > 10) return false;
        const int v = receive_extend(b, s);
        if (dst) dst[kNatural[k]] = (int16_t)v;
        ++k;
    }
    return !b.overrun();
}

inline unsigned be16(const uint8_t* p) { return ((unsigned)p[0] << 8) | p[1]; }

// The marker parse up to and including SOS: everything of `sc` but the interval list.  *entropy: where the
// entropy-coded data begins.  0, or -1 unreadable.
int parse_header(const uint8_t* data, size_t nbytes, JpegScan* sc, size_t* entropy) {
    JpegInfo* info = &sc->info;
    if (!data || nbytes < 4 || data[0] != 0xFF || data[1] != 0xD8) return -1;
    uint16_t qt[4][64];
    bool qt_defined[4] = {false, false, false, false};
    Huff* hd = sc->dc;
    Huff* ha = sc->ac;
    for (int i = 0; i < 4; ++i) hd[i].defined = ha[i].defined = 0;
    int ncomp = 0, comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
    int* comp_h = sc->comp_h;
    int* comp_v = sc->comp_v;
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = -1;
    unsigned restart_interval = 0;
    size_t pos = 2;

    for (;;) {
        // a marker: FF, any number of fill FFs, the code
        if (pos >= nbytes || data[pos] != 0xFF) return -1;
        while (pos < nbytes && data[pos] == 0xFF) ++pos;
        if (pos >= nbytes) return -1;
        const int m = data[pos++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // TEM, a stray RSTn: no parameters
        if (m == 0x00 || m == 0xD8 || m == 0xD9) return -1;   // no marker; a second SOI; EOI before any scan
        if (pos + 2 > nbytes) return -1;
        const size_t len = be16(data + pos);
        if (len < 2 || len > nbytes - pos) return -1;
        const uint8_t* d = data + pos + 2;
        const size_t dl = len - 2;
        pos += len;

        if (m == 0xC0 || m == 0xC1) {  // SOF0 / SOF1: sequential, Huffman
            if (have_sof || dl < 6) return -1;
            const int prec = d[0], h = (int)be16(d + 1), w = (int)be16(d + 3), nc = d[5];
            if (prec != 8 || h == 0 || w == 0 || h > kMaxSide || w > kMaxSide) return -1;  // (h == 0: DNL)
            if ((nc != 1 && nc != 3) || dl != (size_t)(6 + 3 * nc)) return -1;
            for (int c = 0; c < nc; ++c) {
                comp_id[c] = d[6 + 3 * c];
                comp_h[c] = d[7 + 3 * c] >> 4;
                comp_v[c] = d[7 + 3 * c] & 15;
                comp_tq[c] = d[8 + 3 * c];
                if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4 || comp_tq[c] > 3) return -1;
            }
            for (int c = 1; c < nc; ++c)  // luma is the full-resolution plane
                if (comp_h[c] > comp_h[0] || comp_v[c] > comp_v[0]) return -1;
            ncomp = nc;
            info->width = w;
            info->height = h;
            have_sof = true;
        } else if ((m >= 0xC2 && m <= 0xCF && m != 0xC4) || m == 0xDC) {
            return -1;  // progressive, lossless, differential, arithmetic (and DAC, JPG), DNL
        } else if (m == 0xC4) {  // DHT: any number of tables
            size_t q = 0;
            while (q < dl) {
                if (dl - q < 17) return -1;
                const int tc = d[q] >> 4, th = d[q] & 15;
                if (tc > 1 || th > 3) return -1;
                int total = 0;
                for (int i = 0; i < 16; ++i) total += d[q + 1 + i];
                if (total > 256 || dl - q - 17 < (size_t)total) return -1;
                if (!build_huff(tc ? ha[th] : hd[th], d + q + 1, d + q + 17, total)) return -1;
                q += 17 + (size_t)total;
            }
        } else if (m == 0xDB) {  // DQT: any number of tables, 8 or 16 bit, in zigzag order
            size_t q = 0;
            while (q < dl) {
                const int pq = d[q] >> 4, tq = d[q] & 15;
                if (pq > 1 || tq > 3) return -1;
                const size_t need = 1 + (pq ? 128 : 64);
                if (dl - q < need) return -1;
                for (int i = 0; i < 64; ++i)
                    qt[tq][kNatural[i]] = (uint16_t)(pq ? be16(d + q + 1 + 2 * i) : d[q + 1 + i]);
                qt_defined[tq] = true;
                q += need;
            }
        } else if (m == 0xDD) {  // DRI
            if (dl != 2) return -1;
            restart_interval = be16(d);
        } else if (m == 0xE0) {
            if (dl >= 5 && !memcmp(d, "JFIF", 5)) jfif = true;
        } else if (m == 0xEE) {
            if (dl >= 12 && !memcmp(d, "Adobe", 5)) { adobe = true; adobe_transform = d[11]; }
        } else if (m == 0xDA) {  // SOS: the one scan, all components in frame order
            if (!have_sof || dl < 1) return -1;
            const int ns = d[0];
            if (ns != ncomp || dl != (size_t)(4 + 2 * ns)) return -1;
            int* td = sc->td;
            int* ta = sc->ta;
            for (int c = 0; c < ns; ++c) {
                if (d[1 + 2 * c] != comp_id[c]) return -1;
                td[c] = d[2 + 2 * c] >> 4;
                ta[c] = d[2 + 2 * c] & 15;
                if (td[c] > 3 || ta[c] > 3 || !hd[td[c]].defined || !ha[ta[c]].defined) return -1;
            }
            if (d[1 + 2 * ns] != 0 || d[2 + 2 * ns] != 63 || d[3 + 2 * ns] != 0) return -1;  // Ss, Se, Ah/Al
            if (ncomp == 3) {
                // what libjpeg would take for RGB has no luma plane
                if (adobe && adobe_transform == 0) return -1;
                if (!adobe && !jfif && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return -1;
            }
            if (!qt_defined[comp_tq[0]]) return -1;
            memcpy(info->quant, qt[comp_tq[0]], sizeof(info->quant));
            // a single-component scan is not interleaved: one block per MCU whatever its sampling factors say
            const int H0 = ncomp == 1 ? 1 : comp_h[0], V0 = ncomp == 1 ? 1 : comp_v[0];
            if (ncomp == 1) comp_h[0] = comp_v[0] = 1;
            sc->ncomp = ncomp;
            sc->mcus_x = (info->width + 8 * H0 - 1) / (8 * H0);
            sc->mcus_y = (info->height + 8 * V0 - 1) / (8 * V0);
            info->blocks_w = sc->mcus_x * H0;
            info->blocks_h = sc->mcus_y * V0;
            sc->blocks_per_mcu = 0;
            for (int c = 0; c < ncomp; ++c) sc->blocks_per_mcu += comp_h[c] * comp_v[c];
            if (sc->blocks_per_mcu > 10) return -1;  // (the standard's limit)
            sc->restart_interval = restart_interval;
            *entropy = pos;
            return 0;
        }
        // every other segment (APPn, COM, ...) is skipped
    }
}

// a block takes at least two bits: a stream this short cannot hold the frame (and is not walked to find out)
bool too_short(const JpegScan& sc, size_t nbytes, size_t entropy) {
    return (size_t)sc.mcus_x * sc.mcus_y * sc.blocks_per_mcu / 4 > nbytes - entropy;
}

}  // namespace

int jpeg_scan(const uint8_t* data, size_t nbytes, JpegScan* sc) {
    if (!sc) return -1;
    sc->intervals.clear();
    sc->entropy_begin = 0;
    size_t pos = 0;
    if (parse_header(data, nbytes, sc, &pos) || too_short(*sc, nbytes, pos)) return -1;
    sc->entropy_begin = pos;
    if (!sc->restart_interval) return 0;
    const size_t nmcu = (size_t)sc->mcus_x * sc->mcus_y, count = (nmcu + sc->restart_interval - 1) / sc->restart_interval;
    sc->intervals.reserve(2 * count);
    for (size_t i = 0; i < count; ++i) {
        // the interval: up to the first FF that no 00 follows, or the end of the file
        size_t e = pos;
        while (e < nbytes && !(data[e] == 0xFF && !(e + 1 < nbytes && data[e + 1] == 0))) e += data[e] == 0xFF ? 2 : 1;
        sc->intervals.push_back(pos);
        sc->intervals.push_back(e);
        if (i + 1 == count) break;  // what follows the last interval is not examined
        // RSTn, in sequence: FF, any number of FF, D0 + (i & 7)
        while (e < nbytes && data[e] == 0xFF) ++e;
        if (e >= nbytes || data[e] != 0xD0 + (i & 7)) { sc->intervals.clear(); return -1; }
        pos = e + 1;
    }
    return 0;
}

int jpeg_coefficients(const uint8_t* data, size_t nbytes, int16_t* coef, size_t coef_capacity, int row_pitch_blocks,
                      JpegInfo* info) {
    if (!info) return -1;
    // (static-free, on the stack: 8 tables of ~1.4 KB; worker threads decode side by side)
    JpegScan sc;
    size_t pos = 0;
    const int head = parse_header(data, nbytes, &sc, &pos);
    *info = sc.info;  // (unreadable: partly filled)
    if (head) return -1;
    if (!coef) return 0;
    const int ncomp = sc.ncomp, mcus_x = sc.mcus_x, mcus_y = sc.mcus_y, H0 = sc.comp_h[0], V0 = sc.comp_v[0];
    const int *comp_h = sc.comp_h, *comp_v = sc.comp_v, *td = sc.td, *ta = sc.ta;
    const Huff *hd = sc.dc, *ha = sc.ac;
    const unsigned restart_interval = sc.restart_interval;
    const int pitch = row_pitch_blocks > 0 ? row_pitch_blocks : info->blocks_w;
    if (pitch < info->blocks_w || coef_capacity / 64 / (size_t)pitch < (size_t)info->blocks_h) return -2;
    if (too_short(sc, nbytes, pos)) return -1;

    Bits bits;
    bits.p = data + pos;
    bits.end = data + nbytes;
    int pred[3] = {0, 0, 0};
    size_t done = 0;
    unsigned next_rst = 0;
    for (int my = 0; my < mcus_y; ++my)
        for (int mx = 0; mx < mcus_x; ++mx, ++done) {
            if (restart_interval && done && done % restart_interval == 0) {
                // RSTn, in sequence, exactly here: nothing but the last byte's padding bits is left over
                if (bits.n - bits.pad >= 8) return -1;
                const uint8_t* p = bits.p;
                if (p >= bits.end || *p != 0xFF) return -1;
                while (p < bits.end && *p == 0xFF) ++p;
                if (p >= bits.end || *p != 0xD0 + next_rst) return -1;
                next_rst = (next_rst + 1) & 7;
                bits = Bits();
                bits.p = p + 1;
                bits.end = data + nbytes;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < ncomp; ++c)
                for (int v = 0; v < comp_v[c]; ++v)
                    for (int h = 0; h < comp_h[c]; ++h) {
                        int16_t* dst = c ? nullptr : coef + ((size_t)(my * V0 + v) * pitch + (size_t)(mx * H0 + h)) * 64;
                        if (!decode_block(bits, hd[td[c]], ha[ta[c]], &pred[c], dst)) return -1;
                    }
        }
    return 0;
}

void jpeg_lane_setup(const JpegScan& sc, const JpegHuffTable** tables, int* ntables, JpegLaneGeom* g, int blocks_h, int pitch_blocks) {
    memset(g, 0, sizeof(*g));
    *ntables = 0;
    for (int c = 0; c < sc.ncomp; ++c)
        for (int ac = 0; ac < 2; ++ac) {
            const JpegHuffTable* t = ac ? &sc.ac[sc.ta[c]] : &sc.dc[sc.td[c]];
            int s = 0;
            while (s < *ntables && tables[s] != t) ++s;
            if (s == *ntables) tables[(*ntables)++] = t;  // (at most 2 * 3)
            g->slots |= (uint32_t)s << (4 * (ac ? 4 + c : c));
        }
    g->ncomp = sc.ncomp;
    g->H0 = sc.comp_h[0];
    g->V0 = sc.comp_v[0];
    g->mcus_x = sc.mcus_x;
    for (int c = 0; c < sc.ncomp; ++c) g->nblk |= (uint32_t)(sc.comp_h[c] * sc.comp_v[c]) << (8 * c);
    g->blocks_h = blocks_h;
    g->pitch_blocks = pitch_blocks;
}

size_t jpeg_segment_end(const uint8_t* data, size_t nbytes, size_t begin) {
    size_t e = begin;
    while (e < nbytes && !(data[e] == 0xFF && !(e + 1 < nbytes && data[e + 1] == 0))) e += data[e] == 0xFF ? 2 : 1;
    return e;
}

int jpeg_sync_begin(const uint8_t* data, size_t nbytes, int subsequence, JpegSyncState* st) {
    if (!st || subsequence < 8 || subsequence > 1024 || (subsequence & 3)) return -1;
    if (jpeg_scan(data, nbytes, &st->scan)) return -1;
    const JpegScan& sc = st->scan;
    if (sc.restart_interval) return -3;
    const size_t end = jpeg_segment_end(data, nbytes, sc.entropy_begin);
    if (end - sc.entropy_begin >= kJpegSyncMaxStream) return -4;
    st->stream = data + sc.entropy_begin;
    st->len = (uint32_t)(end - sc.entropy_begin);
    st->subsequence = (uint32_t)subsequence;
    st->nsub = (st->len + st->subsequence - 1) / st->subsequence;
    st->total_blocks = (uint32_t)(sc.mcus_x * sc.mcus_y * sc.blocks_per_mcu);
    if (st->nsub == 0) return -1;  // (no data at all: the first symbol overruns)
    const JpegHuffTable* named[kJpegLaneTables] = {};
    jpeg_lane_setup(sc, named, &st->ntables, &st->geom, sc.info.blocks_h, sc.info.blocks_w);
    for (int s = 0; s < st->ntables; ++s) st->tables[s] = *named[s];
    st->spec.resize(st->nsub);
    for (uint32_t i = 0; i < st->nsub; ++i) {
        const uint32_t begin = i * st->subsequence, stop = begin + st->subsequence < st->len ? begin + st->subsequence : st->len;
        const uint64_t entry = i ? jpeg_sync_spec_entry(st->stream, st->len, begin) : jpeg_sync_pack(0, 0, 0);
        jpeg_sync_speculate(st->stream, st->len, stop, entry, st->tables, kNatural, st->geom, &st->spec[i]);
    }
    st->cur = st->spec;
    return 0;
}

bool jpeg_sync_round(JpegSyncState* st) {
    std::vector<JpegSyncRecord> next(st->nsub);  // (a round reads only what the round before it wrote)
    bool changed = false;
    next[0] = st->cur[0];
    for (uint32_t i = 1; i < st->nsub; ++i) {
        const uint32_t begin = i * st->subsequence, stop = begin + st->subsequence < st->len ? begin + st->subsequence : st->len;
        changed |= jpeg_sync_update(st->stream, st->len, stop, st->cur[i - 1], st->cur[i], st->spec[i], st->tables, kNatural, st->geom, &next[i]);
    }
    st->cur.swap(next);
    return changed;
}

int jpeg_sync_finish(const JpegSyncState& st, int16_t* coef, size_t coef_capacity, int row_pitch_blocks) {
    const JpegInfo& info = st.scan.info;
    const int pitch = row_pitch_blocks > 0 ? row_pitch_blocks : info.blocks_w;
    if (!coef || pitch < info.blocks_w || coef_capacity / 64 / (size_t)pitch < (size_t)info.blocks_h) return -2;
    JpegLaneGeom g = st.geom;
    g.pitch_blocks = pitch;
    // the scan: every subsequence's first block and predictors; nothing behind the first failed one is looked at
    std::vector<JpegSyncStart> start(st.nsub);
    uint64_t cum = 0;
    int64_t pred[3] = {0, 0, 0};
    bool dead = false, reached = false;
    for (uint32_t i = 0; i < st.nsub; ++i) {
        const JpegSyncRecord& r = st.cur[i];
        start[i].first_block = dead || cum > st.total_blocks ? st.total_blocks : (uint32_t)cum;
        for (int c = 0; c < 3; ++c) start[i].pred[c] = (int32_t)(pred[c] < -(1 << 30) ? -(1 << 30) : pred[c] > (1 << 30) ? (1 << 30) : pred[c]);
        if (dead) continue;
        const bool fallback = (r.blocks & kJpegSyncFallback) != 0;
        const uint32_t count = fallback ? (r.blocks >> 16) & 0x7FFFu : r.blocks & 0xFFFFu;
        if (cum < st.total_blocks && cum + count >= st.total_blocks) reached = true;
        cum += count;
        for (int c = 0; c < 3; ++c) pred[c] += r.dc[c];
        dead = fallback;
    }
    if (!reached) return -1;
    for (int by = 0; by < info.blocks_h; ++by) memset(coef + (size_t)by * pitch * 64, 0, (size_t)info.blocks_w * 64 * sizeof(int16_t));
    int flags = 0;
    for (uint32_t i = st.nsub; i-- > 0;) {  // (in reverse: the lanes are independent)
        if (start[i].first_block >= st.total_blocks) continue;
        const uint32_t begin = i * st.subsequence, stop = begin + st.subsequence < st.len ? begin + st.subsequence : st.len;
        const uint64_t entry = i ? st.cur[i - 1].exit : jpeg_sync_pack(0, 0, 0);
        if (entry & kJpegSyncFailed) { flags |= 2; continue; }
        JpegSyncRecord unused;
        flags |= jpeg_sync_lane<true>(st.stream, st.len, stop, entry, st.tables, kNatural, g, start[i], st.total_blocks, coef, &unused);
    }
    return (flags & 2) || !(flags & 1) ? -1 : 0;
}

int jpeg_sync_decode(const uint8_t* data, size_t nbytes, int subsequence, int max_rounds, int16_t* coef, size_t coef_capacity,
                     int row_pitch_blocks, JpegInfo* info, int* rounds, size_t* nsubsequences) {
    JpegSyncState st;
    if (rounds) *rounds = -1;
    if (nsubsequences) *nsubsequences = 0;
    const int rc = jpeg_sync_begin(data, nbytes, subsequence, &st);
    if (info) *info = st.scan.info;
    if (rc) return rc;
    if (nsubsequences) *nsubsequences = st.nsub;
    int t = 0;  // update rounds that changed a record
    while (jpeg_sync_round(&st))
        if (++t > max_rounds) return -3;
    if (rounds) *rounds = t;
    return jpeg_sync_finish(st, coef, coef_capacity, row_pitch_blocks);
}

void jpeg_idct_host(const int16_t* coef, int row_pitch_blocks, const JpegInfo& info, uint8_t* out) {
    const int pitch = row_pitch_blocks > 0 ? row_pitch_blocks : info.blocks_w;
    const int bw = (info.width + 7) / 8, bh = (info.height + 7) / 8;
    uint32_t q[64];
    for (int i = 0; i < 64; ++i) q[i] = info.quant[i];
    for (int by = 0; by < bh; ++by)
        for (int bx = 0; bx < bw; ++bx) {
            const int16_t* c = coef + ((size_t)by * pitch + bx) * 64;
            int32_t ws[64];
            for (int k = 0; k < 8; ++k) {  // pass 1: columns, descaled by 11
                uint32_t d[8];
                int32_t o[8];
                for (int r = 0; r < 8; ++r) d[r] = (uint32_t)(int32_t)c[r * 8 + k] * q[r * 8 + k];
                jpeg_idct8<11>(d, o);
                for (int r = 0; r < 8; ++r) ws[r * 8 + k] = o[r];
            }
            const int x0 = bx * 8, nx = info.width - x0 < 8 ? info.width - x0 : 8;
            for (int r = 0; r < 8 && by * 8 + r < info.height; ++r) {  // pass 2: rows, descaled by 18
                uint32_t d[8];
                int32_t o[8];
                for (int k = 0; k < 8; ++k) d[k] = (uint32_t)ws[r * 8 + k];
                jpeg_idct8<18>(d, o);
                uint8_t* px = out + (size_t)(by * 8 + r) * info.width + x0;
                for (int k = 0; k < nx; ++k) {
                    const int32_t v = o[k] + 128;
                    px[k] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
                }
            }
        }
}

}  // namespace mrg
