// Random affine augmentation on the device (beyond the reference): the normalised (B,3,H,W) float32 batch the
// input pipeline made, warped by one 2x3 matrix per image.  A gather: the matrix maps an OUTPUT pixel centre to input coordinates,
// four neighbouring taps are blended bilinearly, and every tap outside the image reads the normalised filler -- so the frame is
// continuous across its border and a coordinate that is not finite is simply filler.
//
// All arithmetic is float32 with every operation rounded on its own (no contraction: the pragma below and build.py's per-file flag),
// in the association include/ssd_gfx950.h states, so that tests/affine_ref.py can restate it bit for bit.
//
// One thread per output pixel does the three channels; x is fastest, so a wave stores 64 contiguous floats of a plane and its taps
// are runs of neighbours in at most a few input rows.  12 bytes read (from cache lines shared with the neighbours) and 12 written per
// pixel: HBM-bound, no LDS.
#include "common.h"
#include <cmath>
#pragma clang fp contract(off)

namespace {

struct WarpArgs {
    const float* in;                 // [B][3][H][W]
    float* out;                      // [B][3][H][W]
    const float* mats;               // [B][6], device copy
    int H, W;
    float fill[3];
};

__global__ __launch_bounds__(256) void affine_warp_kernel(const WarpArgs a) {
    const int b = blockIdx.y;
    const int plane = a.H * a.W;                                 // < 2^31: the entry refuses more
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= plane) return;
    const int oy = (int)(idx / a.W), ox = (int)(idx % a.W);
    const float* m = a.mats + (size_t)b * 6;                     // uniform over the block: scalar loads
    const float fx = (float)ox + 0.5f, fy = (float)oy + 0.5f;
    const float sx = ((m[0] * fx + m[1] * fy) + m[2]) - 0.5f;
    const float sy = ((m[3] * fx + m[4] * fy) + m[5]) - 0.5f;
    const float* src = a.in + (size_t)b * 3 * plane;
    float* dst = a.out + (size_t)b * 3 * plane + idx;
    // NaN compares false: not live.  Nothing is converted to an integer before this guard has passed.
    const bool live = sx > -1.0f && sx < (float)a.W && sy > -1.0f && sy < (float)a.H;
    if (!live) {
        dst[0] = a.fill[0];
        dst[(size_t)plane] = a.fill[1];
        dst[2 * (size_t)plane] = a.fill[2];
        return;
    }
    const float flx = floorf(sx), fly = floorf(sy);              // -1 .. W-1, -1 .. H-1
    const float ax = sx - flx, ay = sy - fly;
    const int x0 = (int)flx, y0 = (int)fly;
    const int x1 = x0 + 1, y1 = y0 + 1;
    const bool in_x0 = x0 >= 0 && x0 < a.W, in_x1 = x1 >= 0 && x1 < a.W;
    const bool in_y0 = y0 >= 0 && y0 < a.H, in_y1 = y1 >= 0 && y1 < a.H;
    const size_t r0 = (size_t)(in_y0 ? y0 : 0) * a.W, r1 = (size_t)(in_y1 ? y1 : 0) * a.W;
    const size_t c0 = (size_t)(in_x0 ? x0 : 0), c1 = (size_t)(in_x1 ? x1 : 0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = src + (size_t)c * plane;
        const float f = a.fill[c];
        const float v00 = in_y0 && in_x0 ? p[r0 + c0] : f;
        const float v01 = in_y0 && in_x1 ? p[r0 + c1] : f;
        const float v10 = in_y1 && in_x0 ? p[r1 + c0] : f;
        const float v11 = in_y1 && in_x1 ? p[r1 + c1] : f;
        const float top = v00 + (v01 - v00) * ax;
        const float bot = v10 + (v11 - v10) * ax;
        dst[(size_t)c * plane] = top + (bot - top) * ay;
    }
}

}  // namespace

extern "C" int ssd_affine_warp_f32(const float* in_nchw, float* out_nchw, const float* mats_dev, const float* mats_host, int B, int H,
                                   int W, const float* fill3_host, void* stream) {
    if (!in_nchw || !out_nchw || !mats_dev || !mats_host || !fill3_host) return SSD_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || B > 65535) return SSD_ERR_BAD_SHAPE;
    if ((long long)H * W >= (1ll << 31)) return SSD_ERR_BAD_SHAPE;
    const uintptr_t bytes = (uintptr_t)B * 3 * (uintptr_t)H * (uintptr_t)W * sizeof(float);
    const uintptr_t pi = reinterpret_cast<uintptr_t>(in_nchw), po = reinterpret_cast<uintptr_t>(out_nchw);
    if (pi < po + bytes && po < pi + bytes) return SSD_ERR_BAD_SHAPE;      // a gather must not read what it writes
    for (long i = 0; i < (long)B * 6; ++i)
        if (!std::isfinite(mats_host[i])) return SSD_ERR_BAD_SHAPE;
    WarpArgs a{};
    a.in = in_nchw; a.out = out_nchw; a.mats = mats_dev; a.H = H; a.W = W;
    for (int c = 0; c < 3; ++c) a.fill[c] = fill3_host[c];
    const long n = (long)H * W;
    hipLaunchKernelGGL(affine_warp_kernel, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, a);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}
