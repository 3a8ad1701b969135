// What csrc/jpeg.hip and csrc/jpeg_split.hip share: the block geometry of an image, the workspace layout in front (coefficient planes
// of all images, then the component planes of all images), the host-side validation of a batch and the launch of the two kernels
// behind the entropy decode.  Internal to the library; the C ABI is include/ssd_gfx950.h.
#pragma once
#include <vector>

#include "common.h"

struct JpegGeom {
    int mcus_w, mcus_h, total_mcus;
    int blocks_w[3], blocks_h[3];
    long n_blocks[3], total_blocks;
};
typedef JpegGeom Geom;

__host__ __device__ inline Geom geom_of(const ssd_jpeg_desc& d) {
    Geom g;
    g.mcus_w = (d.width + 8 * d.h_samp - 1) / (8 * d.h_samp);
    g.mcus_h = (d.height + 8 * d.v_samp - 1) / (8 * d.v_samp);
    g.total_mcus = g.mcus_w * g.mcus_h;
    g.total_blocks = 0;
    for (int c = 0; c < 3; ++c) {
        const bool on = c < d.n_components;
        g.blocks_w[c] = on ? g.mcus_w * (c == 0 ? d.h_samp : 1) : 0;
        g.blocks_h[c] = on ? g.mcus_h * (c == 0 ? d.v_samp : 1) : 0;
        g.n_blocks[c] = (long)g.blocks_w[c] * g.blocks_h[c];
        g.total_blocks += g.n_blocks[c];
    }
    return g;
}

inline bool jpeg_scope_ok(const ssd_jpeg_desc& d) {
    if (d.width < 1 || d.height < 1 || d.width > SSD_JPEG_MAX_DIM || d.height > SSD_JPEG_MAX_DIM) return false;
    if (d.n_components == 1) return d.h_samp == 1 && d.v_samp == 1;
    if (d.n_components != 3) return false;
    return (d.h_samp == 1 && d.v_samp == 1) || (d.h_samp == 2 && (d.v_samp == 1 || d.v_samp == 2));
}

inline size_t jpeg_up256(size_t n) { return (n + 255) & ~(size_t)255; }

// coefficient planes of all images, then the component planes of all images
inline size_t jpeg_layout(const ssd_jpeg_desc* descs, int B, std::vector<int64_t>& coef, std::vector<int64_t>& plane, size_t* coef_bytes) {
    size_t at = 0;
    for (int b = 0; b < B; ++b) { coef[b] = (int64_t)at; at += jpeg_up256((size_t)geom_of(descs[b]).total_blocks * 64 * sizeof(int16_t)); }
    *coef_bytes = at;
    for (int b = 0; b < B; ++b) { plane[b] = (int64_t)at; at += jpeg_up256((size_t)geom_of(descs[b]).total_blocks * 64); }
    return at;
}

struct JpegBatchInfo {       // what the launches need of a validated batch
    size_t layout_bytes, coef_bytes;
    long max_blocks, max_px;
    int max_segments;
};

// Every host-side check of ssd_jpeg_decode_u8 but the workspace size: SSD_OK, or the status the entry returns (csrc/jpeg.hip).
int jpeg_validate_batch(const uint8_t* arena, size_t arena_bytes, const ssd_jpeg_desc* descs_dev, const ssd_jpeg_desc* descs_host,
                        const int32_t* seg_offsets_dev, const int32_t* seg_offsets_host, int n_seg_offsets, int B, const int32_t* status,
                        const void* workspace, int stages, JpegBatchInfo* info);
// the SSD_JPEG_IDCT and SSD_JPEG_COLOUR stages of `stages` (csrc/jpeg.hip)
int jpeg_launch_idct_colour(uint8_t* arena, const ssd_jpeg_desc* descs_dev, int B, const int32_t* status, uint8_t* ws,
                            const JpegBatchInfo& info, int stages, hipStream_t st);
