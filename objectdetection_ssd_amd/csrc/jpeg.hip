// Baseline JPEG decode on the device, into the pixel slots of the input pipeline's arena (include/ssd_gfx950.h, "baseline JPEG
// decode"): what libjpeg's default path -- and so PIL.Image.open(f).convert("RGB") -- computes, bit for bit.  All of it is integer
// arithmetic:
//   1. entropy decode (csrc/jpeg_entropy.h): one workgroup per image builds the image's Huffman tables in LDS, then one LANE per
//      restart segment writes de-zigzagged int16 coefficients into the image's block planes (zeroed by one memset);
//   2. dequantise + jidctint's "islow" IDCT (CONST_BITS 13, PASS1_BITS 2; columns descaled by 11, rows by 18, +128, range limit):
//      eight lanes per block, a column then a row each, the 8 x 8 workspace transposed through LDS;
//   3. jdsample's "fancy" triangle upsampling of chroma on the TRUE down-sampled plane (edge sample / row replicated; nothing of the
//      block padding is read) + jdcolor's 16-bit fixed-point YCbCr -> RGB, one lane per pixel, cropped to width x height.
// A stream can make lanes disagree on how long they run, never on where they may write: see the bounds in jpeg_entropy.h.
#include <algorithm>
#include <utility>
#include <vector>

#include "common.h"
#include "jpeg_common.h"
#include "jpeg_entropy.h"

namespace {

// ---- 1. entropy decode ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void jpeg_entropy_kernel(const uint8_t* __restrict__ arena, const ssd_jpeg_desc* __restrict__ descs,
                                                           const int32_t* __restrict__ seg_offsets, uint8_t* __restrict__ ws,
                                                           int32_t* __restrict__ status) {
    __shared__ JpegHuff tabs[4];
    __shared__ int tab_ok[4];
    __shared__ uint8_t zigzag[64];
    const int b = blockIdx.x;
    const ssd_jpeg_desc& d = descs[b];
    if (threadIdx.x < 4) {
        const int t = threadIdx.x;
        tab_ok[t] = d.n_huffval[t] > 0 && jpeg_huff_build(d.bits[t], d.huffval[t], d.n_huffval[t], &tabs[t]) == 0;
    }
    if (threadIdx.x < 64) zigzag[threadIdx.x] = (uint8_t)jpeg_zigzag(threadIdx.x);
    __syncthreads();
    const Geom g = geom_of(d);
    JpegScan s;
    // the low 32 bits of a generic pointer into LDS are the LDS address
    s.zigzag = reinterpret_cast<const JPEG_LDS uint8_t*>(reinterpret_cast<uintptr_t>(&zigzag[0]));
    s.n_components = d.n_components;
    s.h_samp = d.h_samp;
    s.v_samp = d.v_samp;
    s.mcus_w = g.mcus_w;
    s.total_mcus = g.total_mcus;
    int16_t* plane = reinterpret_cast<int16_t*>(ws + d.coef_offset);
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
        const int td = d.dc_sel[c] & 1, ta = 2 + (d.ac_sel[c] & 1);
        s.coef[c] = plane;
        s.blocks_w[c] = g.blocks_w[c];
        s.dc[c] = reinterpret_cast<const JPEG_LDS JpegHuff*>(reinterpret_cast<uintptr_t>(&tabs[td]));
        s.ac[c] = reinterpret_cast<const JPEG_LDS JpegHuff*>(reinterpret_cast<uintptr_t>(&tabs[ta]));
        plane += g.n_blocks[c] * 64;
        if (c < d.n_components) ok = ok && tab_ok[td] && tab_ok[ta];
    }
    int err;
    const int per = jpeg_segment_mcus(d.n_segments, d.restart_interval, g.total_mcus, &err);
    if (!ok) err |= JPEG_ERR_CODE;                              // the host refuses such a descriptor; never decode with a table not built
    if (err && threadIdx.x == 0) atomicOr(&status[b], err);
    if (!ok) return;
    const int32_t* seg = seg_offsets + d.seg_first;
    const uint8_t* data = arena + d.stream_offset;
    // Segments go to the waves round-robin (segment k to wave k % waves), so that few segments leave ONE lane per wave: lanes of a wave
    // run the decoder's data-dependent branches in lockstep, and every lane less is a serialisation less.
    const int waves = blockDim.x >> 6;
    for (int k = (threadIdx.x & 63) * waves + (threadIdx.x >> 6); k < d.n_segments; k += blockDim.x) {
        const int begin = seg[k], end = jpeg_segment_end(seg, k, d.n_segments, d.stream_bytes);
        const int r = jpeg_decode_segment(data + begin, end - begin, k * per, per, s);
        if (r) atomicOr(&status[b], r);
    }
}

// ---- 2. dequantise + IDCT -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void idct_pass(const int (&v)[8], int (&o)[8], int shift) {
    int z2 = v[2], z3 = v[6];
    int z1 = (z2 + z3) * 4433;                                   // FIX(0.541196100)
    int tmp2 = z1 - z3 * 15137;                                  // FIX(1.847759065)
    int tmp3 = z1 + z2 * 6270;                                   // FIX(0.765366865)
    int tmp0 = (v[0] + v[4]) * 8192, tmp1 = (v[0] - v[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = v[7]; tmp1 = v[5]; tmp2 = v[3]; tmp3 = v[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;                             // FIX(1.175875602)
    tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;   // FIX(0.298631336) (2.053119869) (3.072711026) (1.501321110)
    z1 *= -7373; z2 *= -20995;                                   // FIX(0.899976223) (2.562915447)
    z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;                 // FIX(1.961570560) (0.390180644)
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const int half = 1 << (shift - 1);
    o[0] = (tmp10 + tmp3 + half) >> shift; o[7] = (tmp10 - tmp3 + half) >> shift;
    o[1] = (tmp11 + tmp2 + half) >> shift; o[6] = (tmp11 - tmp2 + half) >> shift;
    o[2] = (tmp12 + tmp1 + half) >> shift; o[5] = (tmp12 - tmp1 + half) >> shift;
    o[3] = (tmp13 + tmp0 + half) >> shift; o[4] = (tmp13 - tmp0 + half) >> shift;
}

// libjpeg's post-IDCT table look-up: clamp(x + 128) for |x| < 512, wrapping modulo 1024 beyond
__device__ __forceinline__ unsigned range_limit(int x) {
    const int i = x & 1023;
    return i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896));
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const ssd_jpeg_desc* __restrict__ descs, uint8_t* __restrict__ ws) {
    __shared__ int tr[32][8][9];
    const ssd_jpeg_desc& d = descs[blockIdx.y];
    const Geom g = geom_of(d);
    const int16_t* coef = reinterpret_cast<const int16_t*>(ws + d.coef_offset);
    uint8_t* planes = ws + d.plane_offset;
    const int lane = threadIdx.x & 7, slot = threadIdx.x >> 3;
    const long groups = (g.total_blocks + 31) / 32;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {            // uniform per workgroup: the barriers are safe
        const long i = grp * 32 + slot;
        const bool on = i < g.total_blocks;
        int c = 0;
        long ic = i, plane_at = 0;
        if (on) {
            while (c < 2 && ic >= g.n_blocks[c]) { ic -= g.n_blocks[c]; plane_at += g.n_blocks[c] * 64; ++c; }
            const uint16_t* q = d.quant[d.quant_sel[c] & 3];
            const int16_t* blk = coef + i * 64;
            int v[8], o[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = (int)blk[r * 8 + lane] * (int)q[r * 8 + lane];
            idct_pass(v, o, 11);
#pragma unroll
            for (int r = 0; r < 8; ++r) tr[slot][r][lane] = o[r];
        }
        __syncthreads();
        if (on) {
            int v[8], o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = tr[slot][lane][j];
            idct_pass(v, o, 18);
            const int by = (int)(ic / g.blocks_w[c]), bx = (int)(ic - (long)by * g.blocks_w[c]);
            const unsigned lo = range_limit(o[0]) | range_limit(o[1]) << 8 | range_limit(o[2]) << 16 | range_limit(o[3]) << 24;
            const unsigned hi = range_limit(o[4]) | range_limit(o[5]) << 8 | range_limit(o[6]) << 16 | range_limit(o[7]) << 24;
            // row (by*8 + lane) of a plane blocks_w*8 wide, 8 bytes at column bx*8: inside the plane since ic < n_blocks[c]
            *reinterpret_cast<uint2*>(planes + plane_at + ((long)(by * 8 + lane) * g.blocks_w[c] + bx) * 8) = make_uint2(lo, hi);
        }
        __syncthreads();
    }
}

// ---- 3. upsample + colour -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jpeg_colour_kernel(uint8_t* __restrict__ arena, const ssd_jpeg_desc* __restrict__ descs,
                                                          const uint8_t* __restrict__ ws, const int32_t* __restrict__ status) {
    const int b = blockIdx.y;
    const ssd_jpeg_desc& d = descs[b];
    const Geom g = geom_of(d);
    const int w = d.width, h = d.height;
    const long n = (long)h * w;                                  // n * 3 <= dst_bytes: checked on the host
    uint8_t* dst = arena + d.dst_offset;
    const bool bad = status[b] != 0;
    const uint8_t* py = ws + d.plane_offset;
    const uint8_t* pcb = py + g.n_blocks[0] * 64;
    const uint8_t* pcr = pcb + g.n_blocks[1] * 64;
    const int wy = g.blocks_w[0] * 8, wc = g.blocks_w[1] * 8;
    const int hs = d.h_samp, vs = d.v_samp;
    const int dw = hs == 2 ? (w + 1) >> 1 : w, dh = vs == 2 ? (h + 1) >> 1 : h;      // the true down-sampled chroma plane
    const bool fancy = dw > 2;                                   // libjpeg replicates narrower planes
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        int r = 0, gg = 0, bl = 0;
        if (!bad) {
            const int y = (int)(i / w), x = (int)(i - (long)y * w);
            const int Y = py[(long)y * wy + x];
            if (d.n_components == 1) {
                r = gg = bl = Y;
            } else {
                int cb, cr;
                if (hs == 1) {
                    cb = pcb[(long)y * wc + x]; cr = pcr[(long)y * wc + x];
                } else if (!fancy) {
                    const long at = (long)(vs == 2 ? y >> 1 : y) * wc + (x >> 1);
                    cb = pcb[at]; cr = pcr[at];
                } else {
                    const int cx = x >> 1;
                    const int ox = (x & 1) ? min(cx + 1, dw - 1) : max(cx - 1, 0);          // the neighbour column, edge replicated
                    if (vs == 1) {
                        const long row = (long)y * wc;
                        const int rnd = (x & 1) ? 2 : 1;
                        cb = (3 * pcb[row + cx] + pcb[row + ox] + rnd) >> 2;
                        cr = (3 * pcr[row + cx] + pcr[row + ox] + rnd) >> 2;
                    } else {
                        const int cy = y >> 1;
                        const int oy = (y & 1) ? min(cy + 1, dh - 1) : max(cy - 1, 0);      // the neighbour row, edge replicated
                        const long r0 = (long)cy * wc, r1 = (long)oy * wc;
                        const int rnd = (x & 1) ? 7 : 8;
                        cb = (3 * (3 * pcb[r0 + cx] + pcb[r1 + cx]) + (3 * pcb[r0 + ox] + pcb[r1 + ox]) + rnd) >> 4;
                        cr = (3 * (3 * pcr[r0 + cx] + pcr[r1 + cx]) + (3 * pcr[r0 + ox] + pcr[r1 + ox]) + rnd) >> 4;
                    }
                }
                cb -= 128; cr -= 128;
                r = Y + ((91881 * cr + 32768) >> 16);                                        // FIX(1.40200)
                gg = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);                         // FIX(0.34414), FIX(0.71414)
                bl = Y + ((116130 * cb + 32768) >> 16);                                      // FIX(1.77200)
                r = min(255, max(0, r)); gg = min(255, max(0, gg)); bl = min(255, max(0, bl));
            }
        }
        dst[3 * i] = (uint8_t)r; dst[3 * i + 1] = (uint8_t)gg; dst[3 * i + 2] = (uint8_t)bl;
    }
}

}  // namespace

extern "C" size_t ssd_jpeg_decode_workspace(ssd_jpeg_desc* descs_host, int B) {
    if (!descs_host || B <= 0 || B > 65535) return 0;
    for (int b = 0; b < B; ++b)
        if (!jpeg_scope_ok(descs_host[b])) return 0;
    std::vector<int64_t> coef(B), plane(B);
    size_t coef_bytes;
    const size_t total = jpeg_layout(descs_host, B, coef, plane, &coef_bytes);
    for (int b = 0; b < B; ++b) { descs_host[b].coef_offset = coef[b]; descs_host[b].plane_offset = plane[b]; }
    return total + 256;
}

int jpeg_validate_batch(const uint8_t* arena, size_t arena_bytes, const ssd_jpeg_desc* descs_dev, const ssd_jpeg_desc* descs_host,
                        const int32_t* seg_offsets_dev, const int32_t* seg_offsets_host, int n_seg_offsets, int B, const int32_t* status,
                        const void* workspace, int stages, JpegBatchInfo* info) {
    if (!arena || !descs_dev || !descs_host || !seg_offsets_dev || !seg_offsets_host || !status || !workspace) return SSD_ERR_NULL;
    if (B <= 0 || B > 65535 || n_seg_offsets <= 0 || stages <= 0 || stages > SSD_JPEG_ALL) return SSD_ERR_BAD_SHAPE;
    if (!ssd_aligned16(workspace)) return SSD_ERR_ALIGN;
    std::vector<int64_t> coef(B), plane(B);
    std::vector<std::pair<int64_t, int64_t>> spans;
    spans.reserve(2 * (size_t)B);
    long max_blocks = 1, max_px = 1;
    int max_segments = 1;
    for (int b = 0; b < B; ++b) {
        const ssd_jpeg_desc& d = descs_host[b];
        if (!jpeg_scope_ok(d)) return SSD_ERR_BAD_SHAPE;
        const Geom g = geom_of(d);
        for (int t = 0; t < 4; ++t) {
            if (d.n_huffval[t] < 0 || d.n_huffval[t] > 256) return SSD_ERR_BAD_SHAPE;
            JpegHuff probe;
            if (d.n_huffval[t] && jpeg_huff_build(d.bits[t], d.huffval[t], d.n_huffval[t], &probe) != 0) return SSD_ERR_BAD_SHAPE;
        }
        for (int c = 0; c < d.n_components; ++c)
            if (d.quant_sel[c] > 3 || d.dc_sel[c] > 1 || d.ac_sel[c] > 1 || d.n_huffval[d.dc_sel[c]] == 0 || d.n_huffval[2 + d.ac_sel[c]] == 0)
                return SSD_ERR_BAD_SHAPE;
        if (d.stream_bytes < 0 || d.stream_offset < 0 || (uint64_t)d.stream_offset + (uint64_t)d.stream_bytes > arena_bytes) return SSD_ERR_BAD_SHAPE;
        if (d.dst_offset < 0 || d.dst_bytes < (int64_t)d.width * d.height * 3 || (uint64_t)d.dst_offset > arena_bytes ||
            (uint64_t)d.dst_bytes > arena_bytes - (uint64_t)d.dst_offset)
            return SSD_ERR_BAD_SHAPE;
        if (d.restart_interval < 0 || d.restart_interval > 65535 || d.n_segments < 1 || d.seg_first < 0 ||
            (long)d.seg_first + d.n_segments > (long)n_seg_offsets)
            return SSD_ERR_BAD_SHAPE;
        const long allowed = d.restart_interval == 0 ? 1 : (g.total_mcus + (long)d.restart_interval - 1) / d.restart_interval;
        if (d.n_segments > allowed) return SSD_ERR_BAD_SHAPE;
        const int32_t* seg = seg_offsets_host + d.seg_first;
        if (seg[0] < 0 || seg[d.n_segments - 1] > d.stream_bytes) return SSD_ERR_BAD_SHAPE;
        for (int k = 0; k + 1 < d.n_segments; ++k)
            if ((long)seg[k + 1] < (long)seg[k] + 2) return SSD_ERR_BAD_SHAPE;
        if (d.stream_bytes) spans.emplace_back(d.stream_offset, d.stream_offset + d.stream_bytes);
        spans.emplace_back(d.dst_offset, d.dst_offset + d.dst_bytes);
        max_blocks = std::max(max_blocks, g.total_blocks);
        max_px = std::max(max_px, (long)d.width * d.height);
        max_segments = std::max(max_segments, (int)d.n_segments);
    }
    std::sort(spans.begin(), spans.end());
    for (size_t i = 0; i + 1 < spans.size(); ++i)
        if (spans[i].second > spans[i + 1].first) return SSD_ERR_BAD_SHAPE;          // a slot over a stream or another slot
    size_t coef_bytes;
    const size_t total = jpeg_layout(descs_host, B, coef, plane, &coef_bytes);
    for (int b = 0; b < B; ++b)
        if (descs_host[b].coef_offset != coef[b] || descs_host[b].plane_offset != plane[b]) return SSD_ERR_BAD_SHAPE;
    info->layout_bytes = total;
    info->coef_bytes = coef_bytes;
    info->max_blocks = max_blocks;
    info->max_px = max_px;
    info->max_segments = max_segments;
    return SSD_OK;
}

int jpeg_launch_idct_colour(uint8_t* arena, const ssd_jpeg_desc* descs_dev, int B, const int32_t* status, uint8_t* ws,
                            const JpegBatchInfo& info, int stages, hipStream_t st) {
    if (stages & SSD_JPEG_IDCT) {
        const int gx = (int)std::min<long>((info.max_blocks + 31) / 32, 512);
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3(gx, B), dim3(256), 0, st, descs_dev, ws);
        SSD_CHECK_LAUNCH();
    }
    if (stages & SSD_JPEG_COLOUR) {
        const int gx = (int)std::min<long>((info.max_px + 255) / 256, 1024);
        hipLaunchKernelGGL(jpeg_colour_kernel, dim3(gx, B), dim3(256), 0, st, arena, descs_dev, ws, status);
        SSD_CHECK_LAUNCH();
    }
    return SSD_OK;
}

extern "C" int ssd_jpeg_decode_u8(uint8_t* arena, size_t arena_bytes, const ssd_jpeg_desc* descs_dev, const ssd_jpeg_desc* descs_host,
                                  const int32_t* seg_offsets_dev, const int32_t* seg_offsets_host, int n_seg_offsets, int B,
                                  int32_t* status, void* workspace, size_t workspace_bytes, int stages, void* stream) {
    JpegBatchInfo info;
    const int bad = jpeg_validate_batch(arena, arena_bytes, descs_dev, descs_host, seg_offsets_dev, seg_offsets_host, n_seg_offsets, B, status,
                                        workspace, stages, &info);
    if (bad != SSD_OK) return bad;
    if (workspace_bytes < info.layout_bytes) return SSD_ERR_WORKSPACE;

    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    if (stages & SSD_JPEG_ENTROPY) {
        if (hipMemsetAsync(status, 0, (size_t)B * sizeof(int32_t), st) != hipSuccess) return SSD_ERR_LAUNCH;
        if (hipMemsetAsync(ws, 0, info.coef_bytes, st) != hipSuccess) return SSD_ERR_LAUNCH;
        const int threads = 64 * std::min(16, info.max_segments);
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(B), dim3(threads), 0, st, arena, descs_dev, seg_offsets_dev, ws, status);
        SSD_CHECK_LAUNCH();
    }
    return jpeg_launch_idct_colour(arena, descs_dev, B, status, ws, info, stages, st);
}
