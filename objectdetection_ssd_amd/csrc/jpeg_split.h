// Baseline JPEG entropy decoding of one restart segment by MANY lanes (Weissenberger & Schmidt, "Accelerating JPEG Decompression on
// GPUs", 2021): Huffman streams self-synchronise, so a decoder that starts at an arbitrary bit soon falls onto the true code
// boundaries.  A segment is de-stuffed into a copy, the copy is cut into subsequences of `subseq_bytes` bytes, and every subsequence is
// walked speculatively; the state at each boundary is then repaired until it stops changing, and the coefficients are written last,
// with known block positions and DC predictors.  The integers written are those of jpeg_decode_segment (jpeg_entropy.h).
// Like jpeg_entropy.h this text is compiled for gfx950 (csrc/jpeg_split.hip) and for the CPU (tools/jpeg_split_host_check.cpp, under
// the host sanitizers): it uses nothing of HIP but the function qualifiers and JPEG_LDS.
//
// Synchronisation state between two symbols: the bit position in the de-stuffed segment, the block slot within the MCU (0 ..
// blocks-per-MCU - 1; it selects the component and so the tables) and the zigzag index k (0 = a DC symbol is next).
// Repair rule: entry[i + 1] := exit[i], and subsequence i + 1 is walked again only when its entry changed; entry[0] is the true start
// of the segment.  An exit that ended in an error is NOT handed down (it would absorb everything behind it): the next subsequence
// keeps its own guess, (its boundary, slot 0, k 0).  By induction subsequence i holds the sequential decoder's state after round i,
// so the rounds are bounded by the subsequence count of the segment, and by nothing else (a stream without end-of-block symbols
// never synchronises and takes that many).
//
// Bounded by construction, whatever the stream holds:
//  * every symbol consumes at least 1 bit; a walk without stores ends at its subsequence's end, at most 31 bits behind it;
//  * a walk with stores ends there too, or -- the last one of a segment -- at the segment's block limit (min(interval, total - first)
//    MCUs), each block taking at most 64 symbols;
//  * a coefficient is stored only at zigzag index <= 63 of a block ordinal in [0, limit), so inside the image's own planes;
//  * four bytes are read at byte positions below the de-stuffed length only, so inside a copy padded by 8 zero bytes; beyond it
//    zero bits are supplied, and a block that CONSUMED such bits is reported (JPEG_ERR_EARLY), as the sequential decoder does;
//  * the de-stuffing rule looks back over one run of FF bytes, never before the segment's first byte.
#pragma once
#include "jpeg_entropy.h"

// ---- de-stuffing: exactly the bytes jpeg_refill drops -- the byte behind a kept FF (unless that FF is the segment's last byte).
// Byte i is dropped iff the maximal run of FF ending at i - 1 inside the segment has odd length.
JPEG_HD bool jpeg_destuff_drop(const uint8_t* seg, int i) {
    int run = 0;
    while (run < i && seg[i - 1 - run] == 0xFF) ++run;
    return (run & 1) != 0;
}

// n bytes of a segment, `drop` = jpeg_destuff_drop of the first of them: -> how many are kept; they are written to dst[0 ..) unless
// dst is null
JPEG_HD int jpeg_destuff_bytes(const uint8_t* bytes, int n, bool drop, uint8_t* dst) {
    int kept = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t v = bytes[i];
        if (!drop) {
            if (dst) dst[kept] = v;
            ++kept;
        }
        drop = !drop && v == 0xFF;
    }
    return kept;
}

// bytes [begin, end) of a segment
JPEG_HD int jpeg_destuff_range(const uint8_t* seg, int begin, int end, uint8_t* dst) {
    return begin < end ? jpeg_destuff_bytes(seg + begin, end - begin, jpeg_destuff_drop(seg, begin), dst) : 0;
}

// ---- synchronisation state
struct JpegSync {
    int pos;                 // bits from the start of the de-stuffed segment
    int slot, k;             // block slot within the MCU, zigzag index of the next symbol (0 = DC)
    int err;                 // 0, or the JPEG_ERR_* that ended the walk
};

JPEG_HD uint64_t jpeg_sync_pack(const JpegSync& s) {
    return (uint64_t)(uint32_t)s.pos | (uint64_t)(s.slot & 255) << 32 | (uint64_t)(s.k & 255) << 40 | (uint64_t)(s.err & 255) << 48;
}
JPEG_HD JpegSync jpeg_sync_unpack(uint64_t w) {
    JpegSync s = {(int)(uint32_t)w, (int)(w >> 32) & 255, (int)(w >> 40) & 255, (int)(w >> 48) & 255};
    return s;
}
JPEG_HD int jpeg_blocks_per_mcu(const JpegScan& s) { return s.n_components == 1 ? 1 : s.h_samp * s.v_samp + 2; }
// subsequences of a segment of `dlen` de-stuffed bytes: a segment shorter than one subsequence is a single lane
JPEG_HD int jpeg_subseq_count(int dlen, int subseq_bytes) { return dlen <= subseq_bytes ? 1 : (dlen + subseq_bytes - 1) / subseq_bytes; }

// ---- bit reader over de-stuffed bytes: no FF test.  JpegBits with p = the copy, end = the de-stuffed length, pos = the next byte to
// load; the position of the next bit is pos * 8 - nbits.  The copy is padded by 8 zero bytes, zero bits are supplied behind it.
JPEG_HD void jpeg_refill_plain(JpegBits& b) {
    if (b.nbits < 32) {
        uint32_t v = 0;
        if (b.pos < b.end) __builtin_memcpy(&v, b.p + b.pos, 4);            // pos + 4 <= end + 3: inside the padding
        b.acc |= (uint64_t)__builtin_bswap32(v) << (32 - b.nbits);
        b.nbits += 32;
        b.pos += 4;
    }
}
JPEG_HD int jpeg_bit_position(const JpegBits& b) { return b.pos * 8 - b.nbits; }

// ---- the walk, with and without coefficient stores
struct JpegWalk {
    JpegSync exit;           // err != 0: the walk ended in that error, and pos, slot, k are never used
    int blocks;              // blocks begun (DC symbols started)
    uint32_t dc[3];          // per component, the sum of the DC differences modulo 2^32
};
struct JpegStore {           // what a storing walk knows beyond its entry
    int first_mcu;           // the segment's first MCU
    int ordinal;             // blocks of the segment begun before this walk
    int limit;               // the segment's block limit
    uint32_t pred[3];        // DC predictors at the entry
    int last;                // the segment's last subsequence: walk on past the end until the limit or an error
};

// block `ordinal` of a segment: MCU first + ordinal / blocks_per_mcu, slot ordinal % blocks_per_mcu
JPEG_HD int16_t* jpeg_block_ptr(const JpegScan& s, int first_mcu, int ordinal, int bpm) {
    const int m = first_mcu + ordinal / bpm, sl = ordinal % bpm;
    const int my = m / s.mcus_w, mx = m - my * s.mcus_w;
    const int nl = bpm == 1 ? 1 : bpm - 2;
    if (sl < nl) {
        const int v = sl / s.h_samp, h = sl - v * s.h_samp;
        return s.coef[0] + ((long)(my * s.v_samp + v) * s.blocks_w[0] + (mx * s.h_samp + h)) * 64;
    }
    return (sl == nl ? s.coef[1] : s.coef[2]) + ((long)my * s.blocks_w[1] + mx) * 64;
}

// Decodes symbols from `entry` while the position is below end_bits (a storing walk with w.last set: until the block limit).
// copy: the segment's de-stuffed bytes, dlen of them, then >= 8 zero bytes.
template <bool STORE>
JPEG_HD JpegWalk jpeg_walk(const uint8_t* copy, int dlen, const JpegSync& entry, int end_bits, const JpegScan& s, const JpegStore& w) {
    const int bpm = jpeg_blocks_per_mcu(s), nl = bpm == 1 ? 1 : bpm - 2;
    JpegWalk r;
    r.exit = entry;
    r.exit.err = 0;
    r.blocks = 0;
    r.dc[0] = r.dc[1] = r.dc[2] = 0;
    int slot = entry.slot, k = entry.k, cur = 0;
    if (entry.pos < 0 || slot < 0 || slot >= bpm || k < 0 || k > 63) {      // no state a walk hands down; never decode from it
        r.exit.err = JPEG_ERR_CODE;
        return r;
    }
    uint32_t p0 = 0, p1 = 0, p2 = 0;
    int16_t* out = nullptr;
    if (STORE) {
        cur = k > 0 ? w.ordinal - 1 : w.ordinal;          // k > 0 continues the block the walk before this one began
        if (cur < 0 || cur >= w.limit) return r;
        if (k == 0 && entry.pos > dlen * 8) return r;     // the block before ended in pad bits: its walk reported that and all ends
        slot = cur % bpm;
        p0 = w.pred[0]; p1 = w.pred[1]; p2 = w.pred[2];
        out = jpeg_block_ptr(s, w.first_mcu, cur, bpm);
    }
    JpegBits b = {copy, entry.pos >> 3, dlen, 0, 0, 0};
    jpeg_refill_plain(b);
    jpeg_consume(b, entry.pos & 7);
    int err = 0;
    for (;;) {
        if (!(STORE && w.last) && jpeg_bit_position(b) >= end_bits) break;
        jpeg_refill_plain(b);
        const int comp = slot < nl ? 0 : slot - nl + 1;
        const JPEG_LDS JpegHuff* t;
        if (k == 0) {
            ++r.blocks;
            t = comp == 0 ? s.dc[0] : (comp == 1 ? s.dc[1] : s.dc[2]);
        } else {
            t = comp == 0 ? s.ac[0] : (comp == 1 ? s.ac[1] : s.ac[2]);
        }
        const int sym = jpeg_symbol(b, *t);
        if (sym < 0 || (k == 0 && sym > 15)) { err = JPEG_ERR_CODE; break; }
        const int sz = k == 0 ? sym : (sym & 15), run = k == 0 ? 0 : (sym >> 4);
        if (k > 0 && sz == 0) {
            k = run == 15 ? k + 16 : 64;                  // ZRL, or end of block
        } else {
            k += run;
            if (k > 63) { err = JPEG_ERR_INDEX; break; }
            const int v = sz ? jpeg_receive_extend(b, sz) : 0;
            if (k == 0) {
                r.dc[0] += comp == 0 ? (uint32_t)v : 0u;
                r.dc[1] += comp == 1 ? (uint32_t)v : 0u;
                r.dc[2] += comp == 2 ? (uint32_t)v : 0u;
                if (STORE) {
                    p0 += comp == 0 ? (uint32_t)v : 0u;
                    p1 += comp == 1 ? (uint32_t)v : 0u;
                    p2 += comp == 2 ? (uint32_t)v : 0u;
                    out[0] = (int16_t)(uint16_t)(comp == 0 ? p0 : (comp == 1 ? p1 : p2));
                }
            } else if (STORE) {
                out[s.zigzag[k] & 63] = (int16_t)v;
            }
            ++k;
        }
        if (k >= 64) {                                     // the block is done
            k = 0;
            slot = slot + 1 == bpm ? 0 : slot + 1;
            if (STORE) {
                if (jpeg_bit_position(b) > dlen * 8) { err = JPEG_ERR_EARLY; break; }      // the sequential rule: pad bits consumed
                if (++cur >= w.limit) break;
                out = jpeg_block_ptr(s, w.first_mcu, cur, bpm);
            }
        }
    }
    r.exit.pos = jpeg_bit_position(b);
    r.exit.slot = slot;
    r.exit.k = k;
    r.exit.err = err;
    return r;
}

// what subsequence j > 0 of a segment starts from until the subsequence before it says otherwise
JPEG_HD JpegSync jpeg_sync_guess(int j, int subseq_bytes) {
    JpegSync g = {j * subseq_bytes * 8, 0, 0, 0};
    return g;
}
// the repair rule: the entry of a subsequence from the exit of the one before it (j > 0)
JPEG_HD JpegSync jpeg_sync_next(const JpegSync& exit_before, int j, int subseq_bytes) {
    return exit_before.err ? jpeg_sync_guess(j, subseq_bytes) : exit_before;
}

// ---- one record per subsequence slot, and what one lane does with it in each pass.  Slots: segment k of an image (k-th of its
// seg_offsets, o_k bytes into the entropy-coded data) owns slots o_k / S + k onwards, one per subsequence; the bases are strictly
// increasing by at least the subsequence count of the segment before (raw length / S + 1 at most), so anyone finds a slot's segment
// from the segment offsets alone.  Slots between the last subsequence of a segment and the next base stay unused (j < 0).
struct JpegSubRec {
    uint64_t entry, exit;    // packed JpegSync
    int32_t blocks;          // of the last walk from `entry`
    uint32_t dc[3];
    int32_t seg, j;          // segment, subsequence within it; j < 0: not in use
    int32_t pre_blocks;      // exclusive scan over the segment's subsequences before this one: blocks begun,
    uint32_t pre_dc[3];      //   DC predictors,
    int32_t pre_bad;         //   exits that ended in an error
    int32_t dirty;           // the entry changed in this round: walk again
};

JPEG_HD int jpeg_split_slot_base(int seg_offset, int k, int subseq_bytes) { return seg_offset / subseq_bytes + k; }
// the last of n_seg segments whose first slot is <= i (segment 0 where there is none: the slot is then below its base)
JPEG_HD int jpeg_split_slot_segment(const int32_t* seg, int n_seg, int i, int subseq_bytes) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jpeg_split_slot_base(seg[mid], mid, subseq_bytes) <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}
JPEG_HD int jpeg_split_end_bits(int j, int subseq_bytes, int dlen) {
    const long e = ((long)j + 1) * subseq_bytes;
    return (int)(e < dlen ? e : dlen) * 8;
}

// a walk without stores from the record's entry to the subsequence's end
JPEG_HD void jpeg_split_walk_item(JpegSubRec& r, const uint8_t* copy, int dlen, int subseq_bytes, const JpegScan& s) {
    const JpegStore none = {0, 0, 0, {0, 0, 0}, 0};
    const JpegWalk w = jpeg_walk<false>(copy, dlen, jpeg_sync_unpack(r.entry), jpeg_split_end_bits(r.j, subseq_bytes, dlen), s, none);
    r.exit = jpeg_sync_pack(w.exit);
    r.blocks = w.blocks;
    r.dc[0] = w.dc[0]; r.dc[1] = w.dc[1]; r.dc[2] = w.dc[2];
    r.dirty = 0;
}

// the repair rule on the record of subsequence j > 0; true if its entry changed
JPEG_HD bool jpeg_split_repair_item(JpegSubRec& r, uint64_t exit_before, int subseq_bytes) {
    const uint64_t e = jpeg_sync_pack(jpeg_sync_next(jpeg_sync_unpack(exit_before), r.j, subseq_bytes));
    if (e == r.entry) return false;
    r.entry = e;
    r.dirty = 1;
    return true;
}

// the write pass of one subsequence: -> 0 or the JPEG_ERR_* it met.  n_sub: subsequences of the segment; per: MCUs per segment.
JPEG_HD int jpeg_split_write_item(const JpegSubRec& r, const uint8_t* copy, int dlen, int n_sub, int subseq_bytes, int per, const JpegScan& s) {
    if (r.j < 0 || r.pre_bad) return 0;
    const int bpm = jpeg_blocks_per_mcu(s);
    const long first = (long)r.seg * per;
    long mcus = s.total_mcus - first;
    if (per < mcus) mcus = per;
    if (mcus <= 0) return 0;
    const JpegStore w = {(int)first, r.pre_blocks, (int)mcus * bpm, {r.pre_dc[0], r.pre_dc[1], r.pre_dc[2]}, r.j == n_sub - 1};
    return jpeg_walk<true>(copy, dlen, jpeg_sync_unpack(r.entry), jpeg_split_end_bits(r.j, subseq_bytes, dlen), s, w).exit.err;
}
