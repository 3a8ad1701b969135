// ATSS matching (atss.hip): what loss.hip needs of it.
#pragma once
#include "common.h"

constexpr int ATSS_MAX_LEVELS = 8;
constexpr int ATSS_MAX_TOPK = 32;

// The prior set by pyramid level, as the kernels receive it (by value: a captured call keeps it)
struct AtssLevels {
    int n_levels, topk;
    int cells[ATSS_MAX_LEVELS], anchors[ATSS_MAX_LEVELS];
};

#pragma GCC visibility push(hidden)
// SSD_OK and `out` filled, or SSD_ERR_NULL (a null array) / SSD_ERR_BAD_SHAPE (topk, n_levels, a level < 1, levels that do not sum to P)
int ssd_internal_atss_levels(int P, int topk, int n_levels, const int* level_cells, const int* level_anchors, AtssLevels& out);
// bytes of the (bs, P) key array, a multiple of 256
size_t ssd_internal_atss_key_bytes(int bs, int P);
// One memset node and the assignment pass: keys[i][p] = (IoU bits << 32) | (0xFFFFFFFF - global box index) of the box prior p of image i
// goes to, 0 for none.  The per-box outputs may be NULL.
int ssd_internal_atss_keys(const float* gt, const int32_t* img_start, int bs, int n_gt, const float* pri, const float* pri_xyxy, int P,
                           const AtssLevels& lv, unsigned long long* keys, int32_t* n_cand, double* mean, double* var, int32_t* n_acc,
                           hipStream_t st);
#pragma GCC visibility pop
