// The segment decoder of csrc/jpeg_entropy.h compiled for the CPU, so that the host sanitizers see the very text the GPU runs:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/jpeg_host_check.cpp -o jpeg_host_check
//     ./jpeg_host_check cases.bin
//
// cases.bin is written by tests/test_jpeg_entropy_host_cpu.py (little-endian):
//     int32 magic 0x4A504743, int32 n_cases, then per case
//     int32 width, height, n_components, h_samp, v_samp, restart_interval, n_segments, stream_bytes, expect
//     int32 dc_sel[3], ac_sel[3]
//     4 x { int32 n_vals, uint8 bits[16], uint8 vals[n_vals] }          tables DC0, DC1, AC0, AC1 (n_vals 0 = absent)
//     int32 seg_offsets[n_segments], uint8 stream[stream_bytes]
//     expect == 0: int16 coefficients of every component's block plane, which the decoder must reproduce with status 0
//     expect == 1: the decoder must return a non-zero status
// Every buffer is a heap block of exactly its size, so a read or write one byte outside it stops the program.
// Prints one line per case ("<index> <status>") and exits 0 only if every case met its expectation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../objectdetection_ssd_amd/csrc/jpeg_entropy.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[2];
    if (!rd(f, head, sizeof head) || head[0] != 0x4A504743 || head[1] < 0) { fprintf(stderr, "bad file\n"); return 2; }
    int failures = 0;
    for (int ci = 0; ci < head[1]; ++ci) {
        int32_t h[9], sel[6];
        if (!rd(f, h, sizeof h) || !rd(f, sel, sizeof sel)) { fprintf(stderr, "case %d: short file\n", ci); return 2; }
        const int width = h[0], height = h[1], nc = h[2], hs = h[3], vs = h[4], ri = h[5], nseg = h[6], nbytes = h[7], expect = h[8];
        if (width < 1 || height < 1 || width > 4096 || height > 4096 || (nc != 1 && nc != 3) || hs < 1 || hs > 2 || vs < 1 || vs > 2 ||
            nseg < 1 || nbytes < 0 || ri < 0) { fprintf(stderr, "case %d: bad header\n", ci); return 2; }
        JpegHuff* tabs = static_cast<JpegHuff*>(malloc(4 * sizeof(JpegHuff)));
        bool have[4] = {false, false, false, false};
        for (int t = 0; t < 4; ++t) {
            int32_t nv;
            uint8_t bits[16];
            if (!rd(f, &nv, 4) || !rd(f, bits, 16) || nv < 0 || nv > 256) { fprintf(stderr, "case %d: bad table\n", ci); return 2; }
            uint8_t* vals = static_cast<uint8_t*>(malloc(nv ? nv : 1));
            if (!rd(f, vals, nv)) return 2;
            if (nv) {
                if (jpeg_huff_build(bits, vals, nv, &tabs[t]) != 0) { fprintf(stderr, "case %d: table %d refused\n", ci, t); return 2; }
                have[t] = true;
            }
            free(vals);
        }
        int32_t* segs = static_cast<int32_t*>(malloc(sizeof(int32_t) * nseg));
        uint8_t* stream = static_cast<uint8_t*>(malloc(nbytes ? nbytes : 1));
        if (!rd(f, segs, sizeof(int32_t) * nseg) || !rd(f, stream, nbytes)) return 2;

        uint8_t* zigzag = static_cast<uint8_t*>(malloc(64));
        for (int k = 0; k < 64; ++k) zigzag[k] = (uint8_t)jpeg_zigzag(k);
        JpegScan s;
        s.zigzag = zigzag;
        s.n_components = nc; s.h_samp = hs; s.v_samp = vs;
        s.mcus_w = (width + 8 * hs - 1) / (8 * hs);
        const int mcus_h = (height + 8 * vs - 1) / (8 * vs);
        s.total_mcus = s.mcus_w * mcus_h;
        size_t blocks[3] = {0, 0, 0}, total_blocks = 0;
        for (int c = 0; c < nc; ++c) {
            s.blocks_w[c] = s.mcus_w * (c == 0 ? hs : 1);
            blocks[c] = (size_t)s.blocks_w[c] * mcus_h * (c == 0 ? vs : 1);
            total_blocks += blocks[c];
            if (sel[c] < 0 || sel[c] > 1 || sel[3 + c] < 0 || sel[3 + c] > 1 || !have[sel[c]] || !have[2 + sel[3 + c]]) {
                fprintf(stderr, "case %d: table selector\n", ci);
                return 2;
            }
            s.dc[c] = &tabs[sel[c]];
            s.ac[c] = &tabs[2 + sel[3 + c]];
        }
        int16_t* coef = static_cast<int16_t*>(calloc(total_blocks * 64, sizeof(int16_t)));
        size_t at = 0;
        for (int c = 0; c < nc; ++c) { s.coef[c] = coef + at * 64; at += blocks[c]; }

        int status = 0;
        const int per = jpeg_segment_mcus(nseg, ri, s.total_mcus, &status);
        for (int k = 0; k < nseg; ++k) {
            const int end = jpeg_segment_end(segs, k, nseg, nbytes);
            if (segs[k] < 0 || end < segs[k] || end > nbytes) { fprintf(stderr, "case %d: segment table\n", ci); return 2; }
            // the segment alone in a block of its own size: nothing of the stream beyond it may be touched
            uint8_t* one = static_cast<uint8_t*>(malloc(end - segs[k] ? end - segs[k] : 1));
            memcpy(one, stream + segs[k], end - segs[k]);
            status |= jpeg_decode_segment(one, end - segs[k], k * per, per, s);
            free(one);
        }
        printf("%d %d\n", ci, status);
        if (expect == 0) {
            std::vector<int16_t> want(total_blocks * 64);
            if (!rd(f, want.data(), want.size() * sizeof(int16_t))) return 2;
            if (status != 0) { fprintf(stderr, "case %d: status %d on a good stream\n", ci, status); ++failures; }
            else if (memcmp(want.data(), coef, want.size() * sizeof(int16_t)) != 0) { fprintf(stderr, "case %d: coefficients differ\n", ci); ++failures; }
        } else if (status == 0) {
            fprintf(stderr, "case %d: status 0 on a corrupt stream\n", ci);
            ++failures;
        }
        free(coef); free(stream); free(segs); free(tabs); free(zigzag);
    }
    fclose(f);
    if (failures) { fprintf(stderr, "%d case(s) failed\n", failures); return 1; }
    printf("OK %d cases\n", head[1]);
    return 0;
}
