// Every function that crosses a file boundary inside the library without being part of the C ABI (include/ssd_gfx950.h), declared
// once: the file that defines one and every file that calls one include this header, so a declaration cannot drift from its definition.
#pragma once
#include "common.h"

struct PooledOut { float* y; uint8_t* argmax; int Ho, Wo; };     // destination of the fused conv -> ReLU -> 2x2/s2 max pool form

// One Winograd convolution F(mo x mo, 3x3) of a map (N,H,W) whose geometry travels beside it: what it reads and writes.  An entry point
// fills in the fields it has and leaves the rest zero; its direction's check (winograd.hip) fills in K and U_rows.
struct WinoConv {
    int mo;                                   // 2 or 4
    const float* in;                          // source tensor (N,H,W,K) ...
    const float* planes;                      // ... or its input planes, already formed: `in` is then not read
    int K;                                    // channels of the source = reduction length of the plane GEMMs (% 32 == 0)
    const float* U;                           // transformed filter [P][U_rows][K] (or its limb planes)
    int U_rows;                               // its rows = the channels produced
    float* out; int ldo;                      // destination (N,H,W,ldo), first U_rows channels ...
    PooledOut pooled;                         // ... or, where pooled.y is set, the pooled destination
    const float* bias;
    const float* mask;                        // ReLU mask of the destination as floats ...
    const unsigned long long* mask_bits;      // ... or as the bit words an input transform wrote
    int relu, accumulate;
    float* planes_keep;                       // where the input planes are to stay (NULL: in the workspace)
    unsigned long long* bits_out;             // where the input transform writes the bits in > 0 (NULL: nowhere)
};

// One direct (implicit-GEMM) convolution, forward or data gradient: what it reads and writes.  An entry point of conv_igemm.hip fills in
// the fields it has and leaves the rest zero; its direction's check fills in w_rows where the entry has none.
enum DirectForm { DIRECT_F32, DIRECT_BF16, DIRECT_X3, DIRECT_HALO1 };     // f32 / bf16 operands of an f32 filter; three bf16 limb
                                                                          // planes; the first of them alone (halo kernel only)
struct DirectConv {
    const ssd_conv_geom* g;
    int dgrad;                                // 0: forward, 1: data gradient
    DirectForm form;
    const float* src;                         // x (N,H,W,Ci), or dy (N,Ho,Wo,ldy)
    const void* w;                            // filter OHWI [w_rows][taps][Ci] (data gradient: IHWO [Ci][taps][Co_pad]) or its limb planes
    int w_rows;                               // rows of a forward filter given as limb planes (else the check's: Co, or Ci)
    const float* bias;
    float* dst;                               // y (N,Ho,Wo,ldy), first Co channels, or dx (N,H,W,Ci)
    int ldy;
    int Co_pad;                               // data gradient: channels of the IHWO filter rows (= ldy)
    const float* mask;                        // data gradient: ReLU mask of dx
    int relu, accumulate;
    void* ws; size_t ws_bytes;                // split-K slab (may be NULL)
};

#pragma GCC visibility push(hidden)
// conv_igemm.hip: the per-launch recorder behind ssd_prof_gemm_begin / _collect.  open returns the slot or -1.
int ssd_internal_prof_open(double flops, int kind, hipStream_t st);
void ssd_internal_prof_close(int slot, hipStream_t st);
// conv_igemm.hip: `nbatch` independent GEMMs out[b][M][N] = a[b][M][K] * w[b][N][K]^T (ksplit > 1: raw partial tiles per K slice)
int ssd_internal_gemm_batched(const float* a, const float* w, float* out, int M, int K, int N, int n_rows, int nbatch, size_t batch_a_elems,
                              size_t batch_w_elems, int ksplit, hipStream_t st);
// gemm_nt.hip: the 128 x 128 LDS-DMA form of the same GEMMs, and whether a problem is one of its
int ssd_internal_gemm_nt_wants(int M, int K, int N, int n_rows, int nbatch);
int ssd_internal_gemm_nt(const float* a, const float* w, float* out, int M, int K, int N, int n_rows, int nbatch, size_t batch_a_elems,
                         size_t batch_w_elems, hipStream_t st);
// gemm_x3.hip: the same GEMMs from three bf16 limbs per operand (w3 from ssd_gemm_x3_split_weights), and the TN split-K form
int ssd_internal_gemm_batched_x3(const float* a, const void* w3, float* out, int M, int K, int N, int n_rows, int nbatch, size_t batch_a_elems,
                                 hipStream_t st);
int ssd_internal_gemm_tn_x3(const float* a, const float* c, float* out, int M, int N, int K, int lda, int ldc, int nbatch, int ksplit,
                            int ksteps_per_split, size_t batch_a, size_t batch_c, hipStream_t st);
// gemm_x3v2.hip: 256 x 256 tiles, two wave groups in ping-pong
int ssd_internal_gemm_batched_x3s(const float* a, const void* w3, float* out, int M, int K, int N, int n_rows, int nbatch, size_t batch_a_elems,
                                  hipStream_t st);
// wino_fused.hip: the plane GEMMs + output transform of one F(4x4) convolution on planes V [36][tiles][c.K] in one kernel, and the
// whole convolution from c.in in one kernel.  (H, W): the map, (TH, TW): its tile grid.
int ssd_internal_wino4_gemm_out(const WinoConv& c, const float* V, int tiles, int H, int W, int TH, int TW, hipStream_t st);
int ssd_internal_wino4_full(const WinoConv& c, int tiles, int H, int W, int TH, int TW, hipStream_t st);
#pragma GCC visibility pop
