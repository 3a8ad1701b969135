// Baseline JPEG entropy decoding of ONE restart segment: bit reader, Huffman decode, DC prediction, AC run/size pairs, de-zigzagged
// int16 coefficients into per-component block planes.  The same text is compiled for gfx950 (csrc/jpeg.hip, one lane per segment)
// and for the CPU (tools/jpeg_host_check.cpp, under the host sanitizers), so it uses nothing of HIP but the function qualifiers and one address-space
// qualifier, both macros that are empty on the CPU.
//
// Bounded by construction, whatever the stream holds:
//  * a byte is never read at or past the segment's end -- zero bits are supplied instead, as libjpeg does, and a segment that had to
//    CONSUME such bits is reported (JPEG_ERR_EARLY);
//  * every refill adds at least 8 bits, every AC iteration advances the coefficient index by at least one, the MCU loop is clamped to
//    the image's MCU count: each loop has a fixed upper trip count;
//  * a coefficient is stored only at zigzag index <= 63 of a block of an MCU below the image's MCU count, so every store lands inside
//    the image's own coefficient planes; table look-ups are masked to the table sizes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ inline
#else
#define JPEG_HD inline
#endif
// The tables a lane reads per symbol live in LDS on the device.  Read through a generic pointer they would be FLAT loads, which retire
// in order with the lane's global stores: every symbol would wait for the coefficient store before it.  So the decoder takes them
// through pointers that name the LDS address space; for the CPU the qualifier is empty and they are ordinary pointers.
#if defined(__HIP_DEVICE_COMPILE__)
#define JPEG_LDS __attribute__((address_space(3)))
#else
#define JPEG_LDS
#endif

enum {
    JPEG_ERR_CODE = 1,       // a bit pattern that is no code of the table, or a DC size above 15
    JPEG_ERR_INDEX = 2,      // an AC run that carries the coefficient index above 63
    JPEG_ERR_EARLY = 4,      // the segment ends before its MCUs are done
    JPEG_ERR_SEGMENTS = 8    // fewer restart segments than the MCU count needs
};

struct JpegHuff {            // one DHT, prepared
    uint16_t fast[512];      // indexed by the next 9 bits: (length << 8) | symbol for codes of <= 9 bits, 0 = a longer code
    int32_t maxcode[17];     // [l] largest code of length l, -1 = none
    int32_t valoff[17];      // [l] huffval index of a code of length l = code + valoff[l]
    uint8_t huffval[256];
};

// bits[l-1] = number of codes of length l (l = 1 .. 16), vals = the symbols in code order.  Returns 0, or -1 for a table that is no
// canonical Huffman code (more than 256 symbols, counts that do not add up to n_vals, a code that does not fit its length).
JPEG_HD int jpeg_huff_build(const uint8_t* bits, const uint8_t* vals, int n_vals, JpegHuff* t) {
    int total = 0;
    for (int l = 0; l < 16; ++l) total += bits[l];
    if (n_vals < 0 || n_vals > 256 || total != n_vals) return -1;
    for (int i = 0; i < 512; ++i) t->fast[i] = 0;
    for (int i = 0; i < 256; ++i) t->huffval[i] = i < n_vals ? vals[i] : 0;
    t->maxcode[0] = -1;
    t->valoff[0] = 0;
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = bits[l - 1];
        if (code + n > (1 << l)) return -1;
        t->valoff[l] = k - code;
        t->maxcode[l] = n ? code + n - 1 : -1;
        if (l <= 9)
            for (int j = 0; j < n; ++j) {
                const int lo = (code + j) << (9 - l), hi = (code + j + 1) << (9 - l);      // hi <= 512 by the check above
                for (int i = lo; i < hi; ++i) t->fast[i] = (uint16_t)((l << 8) | vals[k + j]);
            }
        code = (code + n) << 1;
        k += n;
    }
    return 0;
}

struct JpegBits {
    const uint8_t* p;        // the segment's bytes
    int pos, end;
    uint64_t acc;            // next bit = bit 63; bits below `nbits` are zero
    int nbits;
    int pad;                 // zero bits supplied past the segment's end
};

// Fill to at least 32 bits, what one symbol can take (a code of <= 16 bits and <= 15 more).  Four bytes at a time while they hold no FF
// and lie wholly inside the segment -- ONE load per refill then, not one per byte; otherwise byte by byte, dropping the 00 stuffed
// behind an FF.  At most 4 iterations.
JPEG_HD void jpeg_refill(JpegBits& b) {
    while (b.nbits < 32) {
        if (b.pos + 4 <= b.end) {
            uint32_t v;
            __builtin_memcpy(&v, b.p + b.pos, 4);
            const uint32_t x = ~v;                                       // a zero byte of x is an FF of v
            if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) {
                b.acc |= (uint64_t)__builtin_bswap32(v) << (32 - b.nbits);
                b.nbits += 32;
                b.pos += 4;
                continue;
            }
        }
        uint32_t byte = 0;
        if (b.pos < b.end) {
            byte = b.p[b.pos++];
            if (byte == 0xFF && b.pos < b.end) ++b.pos;
        } else {
            b.pad += 8;
        }
        b.acc |= (uint64_t)byte << (56 - b.nbits);
        b.nbits += 8;
    }
}

JPEG_HD void jpeg_consume(JpegBits& b, int n) { b.acc <<= n; b.nbits -= n; }

// needs >= 16 bits in the buffer; -1 = no such code
JPEG_HD int jpeg_symbol(JpegBits& b, const JPEG_LDS JpegHuff& t) {
    const int look = (int)(b.acc >> 48);
    const int e = t.fast[look >> 7];
    if (e) {
        jpeg_consume(b, e >> 8);
        return e & 255;
    }
    for (int l = 10; l <= 16; ++l) {
        const int code = look >> (16 - l);
        if (code <= t.maxcode[l]) {
            jpeg_consume(b, l);
            return t.huffval[(code + t.valoff[l]) & 255];
        }
    }
    return -1;
}

// s = 1 .. 15 bits as a signed value (F.2.2.1 EXTEND); needs >= s bits in the buffer
JPEG_HD int jpeg_receive_extend(JpegBits& b, int s) {
    const int x = (int)(b.acc >> (64 - s));
    jpeg_consume(b, s);
    return x < (1 << (s - 1)) ? x - (1 << s) + 1 : x;
}

struct JpegScan {            // what a segment decoder needs of its image
    int n_components;        // 1 or 3
    int h_samp, v_samp;      // luma blocks per MCU (1 x 1 for a single component); chroma is 1 x 1
    int mcus_w, total_mcus;
    int16_t* coef[3];        // block planes, zeroed: block (row, col) of component c at coef[c] + (row * blocks_w[c] + col) * 64
    int blocks_w[3];         // = mcus_w * h_samp for luma, mcus_w for chroma
    const JPEG_LDS JpegHuff* dc[3];
    const JPEG_LDS JpegHuff* ac[3];
    const JPEG_LDS uint8_t* zigzag;   // 64 bytes: jpeg_zigzag(0 .. 63)
};

// natural (row-major) index of the k-th coefficient of the stream
JPEG_HD int jpeg_zigzag(int k) {
    const uint8_t nat[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                             62, 63};
    return nat[k & 63];
}

// bytes [0, n_bytes) of `data` are one restart segment that starts at MCU `first_mcu` and holds `n_mcus` MCUs (clamped to the image).
// Returns 0 or one JPEG_ERR_* and stops at the first error.
JPEG_HD int jpeg_decode_segment(const uint8_t* data, int n_bytes, int first_mcu, int n_mcus, const JpegScan& s) {
    if (first_mcu < 0 || n_mcus < 0 || n_bytes < 0) return JPEG_ERR_SEGMENTS;
    int last = s.total_mcus;
    if (n_mcus < last - first_mcu) last = first_mcu + n_mcus;
    JpegBits b = {data, 0, n_bytes, 0, 0, 0};
    int pred[3] = {0, 0, 0};
    for (int m = first_mcu; m < last; ++m) {
        const int my = m / s.mcus_w, mx = m - my * s.mcus_w;
#pragma unroll
        for (int c = 0; c < 3; ++c) {                 // unrolled: the per-component fields stay in registers
            if (c >= s.n_components) break;
            const int hs = c == 0 ? s.h_samp : 1, vs = c == 0 ? s.v_samp : 1;
            const JPEG_LDS JpegHuff& dc = *s.dc[c];
            const JPEG_LDS JpegHuff& ac = *s.ac[c];
            for (int blk = 0; blk < hs * vs; ++blk) {
                const int v = blk / hs, h = blk - v * hs;
                int16_t* out = s.coef[c] + ((long)(my * vs + v) * s.blocks_w[c] + (mx * hs + h)) * 64;
                jpeg_refill(b);
                const int size = jpeg_symbol(b, dc);
                if (size < 0 || size > 15) return JPEG_ERR_CODE;
                if (size) pred[c] = (int)((unsigned)pred[c] + (unsigned)jpeg_receive_extend(b, size));
                out[0] = (int16_t)(uint16_t)(unsigned)pred[c];
                int k = 1;
                while (k < 64) {
                    jpeg_refill(b);
                    const int rs = jpeg_symbol(b, ac);
                    if (rs < 0) return JPEG_ERR_CODE;
                    const int run = rs >> 4, sz = rs & 15;
                    if (sz) {
                        k += run;
                        if (k > 63) return JPEG_ERR_INDEX;
                        out[s.zigzag[k] & 63] = (int16_t)jpeg_receive_extend(b, sz);
                        ++k;
                    } else if (run == 15) {
                        k += 16;
                    } else {
                        break;
                    }
                }
                if (b.pad > b.nbits) return JPEG_ERR_EARLY;
            }
        }
    }
    return 0;
}

// seg_offsets[0 .. n_segments): byte offset of each segment in the entropy-coded data of stream_bytes bytes; a segment ends two bytes
// (its RSTn marker) before the next one begins, the last one where the data end.
JPEG_HD int jpeg_segment_end(const int32_t* seg_offsets, int k, int n_segments, int stream_bytes) {
    return k + 1 < n_segments ? seg_offsets[k + 1] - 2 : stream_bytes;
}

// MCUs per segment; JPEG_ERR_SEGMENTS through *err where the segments cannot cover the image
JPEG_HD int jpeg_segment_mcus(int n_segments, int restart_interval, int total_mcus, int* err) {
    const int per = restart_interval > 0 ? restart_interval : total_mcus;
    *err = (long)n_segments * per < (long)total_mcus ? JPEG_ERR_SEGMENTS : 0;
    return per;
}
