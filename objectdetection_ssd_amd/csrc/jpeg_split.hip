// Entropy decode of baseline JPEG streams WITHOUT restart markers by many lanes per segment (csrc/jpeg_split.h has the algorithm and
// its bounds; include/ssd_gfx950.h, ssd_jpeg_decode_split_u8).  Four kernels in front of the IDCT and colour kernels of csrc/jpeg.hip:
//   plan      one workgroup per image sums what the images before it need: where its copies, lengths and records lie in the workspace;
//   de-stuff  one WAVE per restart segment compacts the segment into a copy without the stuffed bytes, 64 x 16 bytes per step (a lane's
//             16 in one load) with a wave prefix sum over the kept counts, and pads the copy with 16 zero bytes;
//   sync      one workgroup per image builds the image's Huffman tables in LDS (and leaves them in the workspace for the write
//             kernel); lanes take subsequences (looping when there are more than lanes), walk them from their guesses,
//             then repeat the repair rule until an LDS flag, read behind a barrier by every lane, stays clear; then one exclusive scan
//             per segment over (blocks begun, DC sums, exits in error);
//   write     any number of workgroups per image: every lane walks its subsequence again from its final entry, now with its block
//             ordinal and predictors, and stores the coefficients.  A lane with an error before it in its segment does nothing; the
//             lane that meets the first error of a segment inside the image ORs it into status[b].
// Every lane of the sync kernel takes the same number of rounds, at most the slot count of the image.  Records are read and written in
// separate phases of a round (entries from exits, then exits from entries), so the result and the counts do not depend on timing.
#include <algorithm>
#include <cstddef>
#include <vector>

#include "common.h"
#include "jpeg_common.h"
#include "jpeg_split.h"

namespace {

constexpr int kMaxStream = 1 << 27;          // bit positions stay below 2^30

struct SplitPlan {                            // per image, 32 bytes: workspace offsets
    int64_t copy_off, rec_off, dlen_off;
    int32_t n_slots, pad;
};

// segment k's copy lies seg_offset[k] + 16 k bytes into the image's copy area: de-stuffing never grows a segment, the RSTn marker and
// the 16 bytes per segment leave room for 16 zero bytes behind every copy
__host__ __device__ inline long split_copy_bytes(const ssd_jpeg_desc& d) { return ((long)d.stream_bytes + 16L * d.n_segments + 31) & ~15L; }
__host__ __device__ inline long split_slots(const ssd_jpeg_desc& d, int S) { return (long)d.stream_bytes / S + d.n_segments + 1; }
__device__ __forceinline__ long split_copy_at(int seg_offset, int k) { return (long)seg_offset + 16L * k; }

__device__ __forceinline__ long wave_sum_l(long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void jpeg_split_plan_kernel(const ssd_jpeg_desc* __restrict__ descs, uint8_t* __restrict__ ws, long plan_off,
                                                              long dlen_off, long rec_off, long copy_off, int S) {
    __shared__ long part[3][4];
    const int b = blockIdx.x;
    long c = 0, r = 0, n = 0;
    for (int i = threadIdx.x; i < b; i += 256) {
        c += split_copy_bytes(descs[i]);
        r += split_slots(descs[i], S);
        n += descs[i].n_segments;
    }
    c = wave_sum_l(c); r = wave_sum_l(r); n = wave_sum_l(n);
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = c; part[1][threadIdx.x >> 6] = r; part[2][threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        SplitPlan p;
        p.copy_off = copy_off + part[0][0] + part[0][1] + part[0][2] + part[0][3];
        p.rec_off = rec_off + (part[1][0] + part[1][1] + part[1][2] + part[1][3]) * (long)sizeof(JpegSubRec);
        p.dlen_off = dlen_off + (part[2][0] + part[2][1] + part[2][2] + part[2][3]) * 4;
        p.n_slots = (int)split_slots(descs[b], S);
        p.pad = 0;
        reinterpret_cast<SplitPlan*>(ws + plan_off)[b] = p;
    }
}

// ---- de-stuff: grid (x, B), 4 waves per workgroup, segments to waves round-robin
__global__ __launch_bounds__(256) void jpeg_split_destuff_kernel(const uint8_t* __restrict__ arena, const ssd_jpeg_desc* __restrict__ descs,
                                                                 const int32_t* __restrict__ seg_offsets, uint8_t* __restrict__ ws, long plan_off) {
    const int b = blockIdx.y;
    const ssd_jpeg_desc& d = descs[b];
    const SplitPlan pl = reinterpret_cast<const SplitPlan*>(ws + plan_off)[b];
    const int32_t* seg = seg_offsets + d.seg_first;
    int32_t* dlen = reinterpret_cast<int32_t*>(ws + pl.dlen_off);
    const int lane = threadIdx.x & 63, waves = gridDim.x * 4;
    for (int k = blockIdx.x * 4 + (threadIdx.x >> 6); k < d.n_segments; k += waves) {      // wave-uniform
        const int begin = seg[k], n = jpeg_segment_end(seg, k, d.n_segments, d.stream_bytes) - begin;
        const uint8_t* src = arena + d.stream_offset + begin;
        uint8_t* dst = ws + pl.copy_off + split_copy_at(begin, k);
        int base = 0;
        for (int t0 = 0; t0 < n; t0 += 1024) {
            const int lo = t0 + lane * 16, hi = min(lo + 16, n);
            // the lane's 16 bytes in one load where they are whole (every byte load of its own would wait for the one before)
            uint8_t own[16];
            const bool whole = lo + 16 <= n;
            if (whole) __builtin_memcpy(own, src + lo, 16);
            const bool drop = lo < hi && jpeg_destuff_drop(src, lo);
            const int cnt = whole ? jpeg_destuff_bytes(own, 16, drop, nullptr) : (lo < hi ? jpeg_destuff_bytes(src + lo, hi - lo, drop, nullptr) : 0);
            int incl = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            uint8_t* to = dst + base + incl - cnt;                                            // base + incl <= hi <= n: inside the copy
            if (whole) jpeg_destuff_bytes(own, 16, drop, to);
            else if (lo < hi) jpeg_destuff_bytes(src + lo, hi - lo, drop, to);
            base += __shfl(incl, 63, 64);
        }
        if (lane < 16) dst[base + lane] = 0;                                                  // base <= n: the padding's room
        if (lane == 0) dlen[k] = base;
    }
}

// ---- what the sync and write kernels share: the image's tables in LDS, its scan description
struct SplitShared {
    JpegHuff tabs[4];
    int tab_ok[4];
    uint8_t zigzag[64];
    uint32_t raw[272];                        // the descriptor's bits[4][16] and huffval[4][256]
};
static_assert(offsetof(ssd_jpeg_desc, huffval) == offsetof(ssd_jpeg_desc, bits) + 64 && offsetof(ssd_jpeg_desc, bits) % 4 == 0 &&
              sizeof(ssd_jpeg_desc) % 4 == 0, "the Huffman tables of a descriptor are 272 aligned words");

constexpr int kTableWords = (4 * (int)sizeof(JpegHuff) + 16) / 4;      // tabs and tab_ok, as they lie at the head of SplitShared
static_assert(offsetof(SplitShared, tab_ok) == 4 * sizeof(JpegHuff) && sizeof(JpegHuff) % 4 == 0, "tabs, then tab_ok");

// All lanes of the workgroup: the image's tables built in LDS and left in the workspace for the write kernel.  The table bytes go to LDS
// first, all lanes: jpeg_huff_build reads them one by one, each read waiting for the one before, and from global memory that alone
// was some 170 us per workgroup.
__device__ __forceinline__ void split_build_tables(const ssd_jpeg_desc& d, SplitShared* sh, uint32_t* keep) {
    const uint32_t* words = reinterpret_cast<const uint32_t*>(&d.bits[0][0]);
    for (int i = threadIdx.x; i < 272; i += blockDim.x) sh->raw[i] = words[i];
    if (threadIdx.x < 64) sh->zigzag[threadIdx.x] = (uint8_t)jpeg_zigzag(threadIdx.x);
    __syncthreads();
    if (threadIdx.x < 4) {
        const int t = threadIdx.x;
        const uint8_t* raw = reinterpret_cast<const uint8_t*>(sh->raw);
        sh->tab_ok[t] = d.n_huffval[t] > 0 && d.n_huffval[t] <= 256 && jpeg_huff_build(raw + 16 * t, raw + 64 + 256 * t, d.n_huffval[t], &sh->tabs[t]) == 0;
    }
    __syncthreads();
    const uint32_t* built = reinterpret_cast<const uint32_t*>(sh);
    for (int i = threadIdx.x; i < kTableWords; i += blockDim.x) keep[i] = built[i];
}

// all lanes of the workgroup: the tables the sync kernel built, from the workspace
__device__ __forceinline__ void split_fetch_tables(SplitShared* sh, const uint32_t* kept) {
    uint32_t* into = reinterpret_cast<uint32_t*>(sh);
    for (int i = threadIdx.x; i < kTableWords; i += blockDim.x) into[i] = kept[i];
    if (threadIdx.x < 64) sh->zigzag[threadIdx.x] = (uint8_t)jpeg_zigzag(threadIdx.x);
    __syncthreads();
}

// with the tables in LDS: -> false for a descriptor the host refuses (a table that is no code)
__device__ __forceinline__ bool split_scan(const ssd_jpeg_desc& d, uint8_t* ws, SplitShared* sh, JpegScan& s, Geom& g) {
    g = geom_of(d);
    // the low 32 bits of a generic pointer into LDS are the LDS address
    s.zigzag = reinterpret_cast<const JPEG_LDS uint8_t*>(reinterpret_cast<uintptr_t>(&sh->zigzag[0]));
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
        s.dc[c] = reinterpret_cast<const JPEG_LDS JpegHuff*>(reinterpret_cast<uintptr_t>(&sh->tabs[td]));
        s.ac[c] = reinterpret_cast<const JPEG_LDS JpegHuff*>(reinterpret_cast<uintptr_t>(&sh->tabs[ta]));
        plane += g.n_blocks[c] * 64;
        if (c < d.n_components) ok = ok && sh->tab_ok[td] && sh->tab_ok[ta];
    }
    return ok;
}

// ---- synchronise: one workgroup per image
__global__ __launch_bounds__(1024) void jpeg_split_sync_kernel(const ssd_jpeg_desc* __restrict__ descs, const int32_t* __restrict__ seg_offsets,
                                                               uint8_t* __restrict__ ws, int32_t* __restrict__ status, long plan_off, int S,
                                                               int32_t* __restrict__ stats, long tab_off) {
    __shared__ SplitShared sh;
    __shared__ int changed, n_walks, n_active;
    __shared__ uint32_t scan_v[5 * 1024];
    __shared__ int scan_h[1024];
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const ssd_jpeg_desc& d = descs[b];
    if (tid == 0) { n_walks = 0; n_active = 0; }
    JpegScan s;
    Geom g;
    split_build_tables(d, &sh, reinterpret_cast<uint32_t*>(ws + tab_off) + (size_t)b * kTableWords);
    const bool ok = split_scan(d, ws, &sh, s, g);
    int err;
    jpeg_segment_mcus(d.n_segments, d.restart_interval, g.total_mcus, &err);
    if (!ok) err |= JPEG_ERR_CODE;                               // the host refuses such a descriptor; never decode with a table not built
    if (err && tid == 0) atomicOr(&status[b], err);
    if (!ok) {
        if (stats && tid < 4) stats[b * 4 + tid] = 0;
        return;
    }
    const SplitPlan pl = reinterpret_cast<const SplitPlan*>(ws + plan_off)[b];
    JpegSubRec* recs = reinterpret_cast<JpegSubRec*>(ws + pl.rec_off);
    const int32_t* dlen = reinterpret_cast<const int32_t*>(ws + pl.dlen_off);
    const uint8_t* copies = ws + pl.copy_off;
    const int32_t* seg = seg_offsets + d.seg_first;
    const int n_slots = pl.n_slots, n_seg = d.n_segments;
    // Slots go to the waves round-robin (slot i to wave i % waves), so that few slots leave one lane per wave.
    const int waves = T >> 6, first = (tid & 63) * waves + (tid >> 6);
    int walks = 0, active = 0;
    // round 0: every subsequence from its guess, the first one of a segment from the true start
    for (int i = first; i < n_slots; i += T) {
        const int k = jpeg_split_slot_segment(seg, n_seg, i, S);
        const int j = i - jpeg_split_slot_base(seg[k], k, S), dl = dlen[k];
        const bool on = j >= 0 && j < jpeg_subseq_count(dl, S);
        JpegSubRec r;
        r.entry = on && j > 0 ? jpeg_sync_pack(jpeg_sync_guess(j, S)) : 0;
        r.exit = 0;
        r.blocks = 0;
        r.dc[0] = r.dc[1] = r.dc[2] = 0;
        r.seg = k;
        r.j = on ? j : -1;
        r.pre_blocks = 0;
        r.pre_dc[0] = r.pre_dc[1] = r.pre_dc[2] = 0;
        r.pre_bad = 0;
        r.dirty = 0;
        if (on) {
            jpeg_split_walk_item(r, copies + split_copy_at(seg[k], k), dl, S, s);
            ++walks;
            ++active;
        }
        recs[i] = r;
    }
    __syncthreads();

    int rounds = 0;
    for (;;) {
        if (tid == 0) changed = 0;
        __syncthreads();
        for (int i = first; i < n_slots; i += T)                 // entries from the exits of the round before
            if (recs[i].j > 0 && jpeg_split_repair_item(recs[i], recs[i - 1].exit, S)) changed = 1;
        __syncthreads();
        const int c = changed;                                   // the same value in every lane of the workgroup
        if (!c || rounds >= n_slots) break;
        ++rounds;
        for (int i = first; i < n_slots; i += T) {               // exits from the entries that changed
            if (recs[i].j < 0 || !recs[i].dirty) continue;
            const int k = recs[i].seg;
            jpeg_split_walk_item(recs[i], copies + split_copy_at(seg[k], k), dlen[k], S, s);
            ++walks;
        }
        __syncthreads();
    }
    atomicAdd(&n_walks, walks);
    atomicAdd(&n_active, active);

    // exclusive scan per segment: lane t holds the slots [t q, (t + 1) q), a slot with j <= 0 starts anew
    const int q = (n_slots + T - 1) / T, lo = min(tid * q, n_slots), hi = min(lo + q, n_slots);
    uint32_t a[5] = {0, 0, 0, 0, 0};
    int head = 0;
    for (int i = lo; i < hi; ++i) {
        const JpegSubRec& r = recs[i];
        const uint32_t v[5] = {(uint32_t)r.blocks, r.dc[0], r.dc[1], r.dc[2], r.j >= 0 && ((r.exit >> 48) & 255) != 0 ? 1u : 0u};
        if (r.j <= 0) head = 1;
#pragma unroll
        for (int e = 0; e < 5; ++e) a[e] = r.j <= 0 ? v[e] : a[e] + v[e];
    }
#pragma unroll
    for (int e = 0; e < 5; ++e) scan_v[e * T + tid] = a[e];
    scan_h[tid] = head;
    __syncthreads();
    for (int o = 1; o < T; o <<= 1) {                            // uniform trip count
        uint32_t p[5] = {0, 0, 0, 0, 0};
        int ph = 0;
        if (tid >= o) {
#pragma unroll
            for (int e = 0; e < 5; ++e) p[e] = scan_v[e * T + tid - o];
            ph = scan_h[tid - o];
        }
        __syncthreads();
        if (tid >= o) {
#pragma unroll
            for (int e = 0; e < 5; ++e) { if (!head) a[e] += p[e]; scan_v[e * T + tid] = a[e]; }
            head |= ph;
            scan_h[tid] = head;
        }
        __syncthreads();
    }
    uint32_t run[5] = {0, 0, 0, 0, 0};
    if (tid > 0) {
#pragma unroll
        for (int e = 0; e < 5; ++e) run[e] = scan_v[e * T + tid - 1];
    }
    for (int i = lo; i < hi; ++i) {
        JpegSubRec& r = recs[i];
        if (r.j <= 0) run[0] = run[1] = run[2] = run[3] = run[4] = 0;
        r.pre_blocks = (int32_t)run[0];
        r.pre_dc[0] = run[1]; r.pre_dc[1] = run[2]; r.pre_dc[2] = run[3];
        r.pre_bad = (int32_t)run[4];
        run[0] += (uint32_t)r.blocks; run[1] += r.dc[0]; run[2] += r.dc[1]; run[3] += r.dc[2];
        run[4] += r.j >= 0 && ((r.exit >> 48) & 255) != 0 ? 1u : 0u;
    }
    if (stats && tid == 0) {                                     // the barriers of the scan are behind the two atomic adds
        stats[b * 4 + 0] = n_active;
        stats[b * 4 + 1] = rounds;
        stats[b * 4 + 2] = n_walks;
        stats[b * 4 + 3] = 0;
    }
}

// ---- write: grid (x, B), 4 waves per workgroup, slots to all waves of the image round-robin
__global__ __launch_bounds__(256) void jpeg_split_write_kernel(const ssd_jpeg_desc* __restrict__ descs, const int32_t* __restrict__ seg_offsets,
                                                               uint8_t* __restrict__ ws, int32_t* __restrict__ status, long plan_off, int S,
                                                               long tab_off) {
    __shared__ SplitShared sh;
    const int b = blockIdx.y;
    const ssd_jpeg_desc& d = descs[b];
    JpegScan s;
    Geom g;
    split_fetch_tables(&sh, reinterpret_cast<const uint32_t*>(ws + tab_off) + (size_t)b * kTableWords);
    if (!split_scan(d, ws, &sh, s, g)) return;
    int err;
    const int per = jpeg_segment_mcus(d.n_segments, d.restart_interval, g.total_mcus, &err);
    const SplitPlan pl = reinterpret_cast<const SplitPlan*>(ws + plan_off)[b];
    const JpegSubRec* recs = reinterpret_cast<const JpegSubRec*>(ws + pl.rec_off);
    const int32_t* dlen = reinterpret_cast<const int32_t*>(ws + pl.dlen_off);
    const uint8_t* copies = ws + pl.copy_off;
    const int32_t* seg = seg_offsets + d.seg_first;
    const int waves = gridDim.x * 4;
    for (long i = (long)(threadIdx.x & 63) * waves + blockIdx.x * 4 + (threadIdx.x >> 6); i < pl.n_slots; i += (long)waves * 64) {
        const JpegSubRec r = recs[i];
        if (r.j < 0 || r.pre_bad) continue;
        const int k = r.seg, dl = dlen[k];
        const int e = jpeg_split_write_item(r, copies + split_copy_at(seg[k], k), dl, jpeg_subseq_count(dl, S), S, per, s);
        if (e) atomicOr(&status[b], e);
    }
}

struct Tail {
    size_t plan_off, tab_off, dlen_off, rec_off, copy_off, total;
    long max_slots;
};

// behind the layout of csrc/jpeg.hip: the plans, the built Huffman tables, the de-stuffed lengths, the records, the copies.  false: outside the scope
bool tail_layout(const ssd_jpeg_desc* descs, int B, int S, size_t front, Tail* t) {
    size_t segs = 0, slots = 0, copies = 0;
    t->max_slots = 1;
    for (int b = 0; b < B; ++b) {
        const ssd_jpeg_desc& d = descs[b];
        if (d.n_segments < 1 || d.stream_bytes < 0 || d.stream_bytes > kMaxStream) return false;
        segs += (size_t)d.n_segments;
        slots += (size_t)split_slots(d, S);
        copies += (size_t)split_copy_bytes(d);
        t->max_slots = std::max(t->max_slots, split_slots(d, S));
    }
    size_t at = jpeg_up256(front);
    t->plan_off = at; at += jpeg_up256((size_t)B * sizeof(SplitPlan));
    t->tab_off = at; at += jpeg_up256((size_t)B * kTableWords * 4);
    t->dlen_off = at; at += jpeg_up256(segs * sizeof(int32_t));
    t->rec_off = at; at += jpeg_up256(slots * sizeof(JpegSubRec));
    t->copy_off = at; at += jpeg_up256(copies);
    t->total = at;
    return true;
}

bool subseq_ok(int S) { return S >= 8 && S <= 4096 && S % 4 == 0; }

}  // namespace

static_assert(sizeof(JpegSubRec) == 64 && sizeof(SplitPlan) == 32, "workspace records");

extern "C" size_t ssd_jpeg_decode_split_workspace(ssd_jpeg_desc* descs_host, int B, const int32_t* seg_offsets_host, int n_seg_offsets,
                                                  int subseq_bytes) {
    if (!descs_host || !seg_offsets_host || B <= 0 || B > 65535 || n_seg_offsets <= 0 || !subseq_ok(subseq_bytes)) return 0;
    for (int b = 0; b < B; ++b) {
        const ssd_jpeg_desc& d = descs_host[b];
        if (!jpeg_scope_ok(d) || d.n_segments < 1 || d.seg_first < 0 || (long)d.seg_first + d.n_segments > (long)n_seg_offsets) return 0;
    }
    std::vector<int64_t> coef(B), plane(B);
    size_t coef_bytes;
    const size_t front = jpeg_layout(descs_host, B, coef, plane, &coef_bytes);
    Tail t;
    if (!tail_layout(descs_host, B, subseq_bytes, front, &t)) return 0;
    for (int b = 0; b < B; ++b) { descs_host[b].coef_offset = coef[b]; descs_host[b].plane_offset = plane[b]; }
    return t.total + 256;
}

extern "C" int ssd_jpeg_decode_split_u8(uint8_t* arena, size_t arena_bytes, const ssd_jpeg_desc* descs_dev, const ssd_jpeg_desc* descs_host,
                                        const int32_t* seg_offsets_dev, const int32_t* seg_offsets_host, int n_seg_offsets, int B,
                                        int32_t* status, void* workspace, size_t workspace_bytes, int stages, void* stream, int subseq_bytes,
                                        int32_t* stats) {
    JpegBatchInfo info;
    const int bad = jpeg_validate_batch(arena, arena_bytes, descs_dev, descs_host, seg_offsets_dev, seg_offsets_host, n_seg_offsets, B, status,
                                        workspace, stages, &info);
    if (bad != SSD_OK) return bad;
    if (!subseq_ok(subseq_bytes)) return SSD_ERR_BAD_SHAPE;
    Tail t;
    if (!tail_layout(descs_host, B, subseq_bytes, info.layout_bytes, &t)) return SSD_ERR_BAD_SHAPE;
    if (workspace_bytes < t.total) return SSD_ERR_WORKSPACE;

    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    if (stages & SSD_JPEG_ENTROPY) {
        if (hipMemsetAsync(status, 0, (size_t)B * sizeof(int32_t), st) != hipSuccess) return SSD_ERR_LAUNCH;
        if (hipMemsetAsync(ws, 0, info.coef_bytes, st) != hipSuccess) return SSD_ERR_LAUNCH;
        hipLaunchKernelGGL(jpeg_split_plan_kernel, dim3(B), dim3(256), 0, st, descs_dev, ws, (long)t.plan_off, (long)t.dlen_off, (long)t.rec_off,
                           (long)t.copy_off, subseq_bytes);
        SSD_CHECK_LAUNCH();
        const int gd = std::min(64, std::max(1, (info.max_segments + 3) / 4));
        hipLaunchKernelGGL(jpeg_split_destuff_kernel, dim3(gd, B), dim3(256), 0, st, arena, descs_dev, seg_offsets_dev, ws, (long)t.plan_off);
        SSD_CHECK_LAUNCH();
        const int threads = 64 * (int)std::min<long>(16, t.max_slots);
        hipLaunchKernelGGL(jpeg_split_sync_kernel, dim3(B), dim3(threads), 0, st, descs_dev, seg_offsets_dev, ws, status, (long)t.plan_off,
                           subseq_bytes, stats, (long)t.tab_off);
        SSD_CHECK_LAUNCH();
        const int gw = (int)std::min<long>(64, std::max<long>(1, (t.max_slots + 15) / 16));
        hipLaunchKernelGGL(jpeg_split_write_kernel, dim3(gw, B), dim3(256), 0, st, descs_dev, seg_offsets_dev, ws, status, (long)t.plan_off,
                           subseq_bytes, (long)t.tab_off);
        SSD_CHECK_LAUNCH();
    }
    return jpeg_launch_idct_colour(arena, descs_dev, B, status, ws, info, stages, st);
}
