// The many-lanes-per-segment decoder of csrc/jpeg_split.h compiled for the CPU, the lanes of csrc/jpeg_split.hip emulated in loops, so
// that the host sanitizers see the very text the GPU runs:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/jpeg_split_host_check.cpp -o jpeg_split_host_check
//     ./jpeg_split_host_check cases.bin 8,12,32,128,256
//
// cases.bin has the format of tools/jpeg_host_check.cpp (written by tests/test_jpeg_split_host_cpu.py).  First the de-stuffing rule is
// held to a byte-serial restatement of jpeg_refill's on seeded random strings rich in FF (lengths 0 .. 300, whole and in chunks).
// Then every case runs at every subsequence size: de-stuff in steps of 64 x 16 bytes, walk, repair until nothing changes, scan, write.
// Required: the status equals jpeg_decode_segment's on the same stream; on a good stream it is 0 and the coefficients equal both the
// file's and jpeg_decode_segment's; the repair rounds do not exceed the subsequence count.  Every buffer is a heap block of exactly its
// size (a copy: its de-stuffed length + 8), so a read or write one byte outside it stops the program.
// Prints "<case> <subseq_bytes> <status> <subsequences> <rounds> <walks>" per run and exits 0 only if every requirement held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../objectdetection_ssd_amd/csrc/jpeg_split.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static int destuff_self_test() {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    int bad = 0;
    for (int len = 0; len <= 300; ++len)
        for (int rep = 0; rep < 8; ++rep) {
            uint8_t* s = static_cast<uint8_t*>(malloc(len ? len : 1));
            for (int i = 0; i < len; ++i) {
                x = x * 6364136223846793005ull + 1442695040888963407ull;
                const int r = (int)(x >> 33) & 7;
                s[i] = r < 3 ? 0xFF : (r == 3 ? 0x00 : (uint8_t)(x >> 40));
            }
            std::vector<uint8_t> want;                           // jpeg_refill's rule, byte by byte
            std::vector<char> kept(len, 0);
            for (int pos = 0; pos < len;) {
                const uint8_t v = s[pos];
                kept[pos++] = 1;
                want.push_back(v);
                if (v == 0xFF && pos < len) ++pos;
            }
            for (int i = 0; i < len; ++i)
                if (jpeg_destuff_drop(s, i) == (kept[i] != 0)) ++bad;
            for (int chunk : {1, 2, 3, 16, 64, 301}) {
                uint8_t* out = static_cast<uint8_t*>(malloc(want.size() ? want.size() : 1));
                size_t at = 0;
                for (int lo = 0; lo < len; lo += chunk) {
                    const int hi = lo + chunk < len ? lo + chunk : len;
                    const int n = jpeg_destuff_range(s, lo, hi, nullptr);
                    if (at + n > want.size()) { ++bad; break; }
                    if (jpeg_destuff_range(s, lo, hi, out + at) != n) ++bad;
                    at += n;
                }
                if (at != want.size() || (at && memcmp(out, want.data(), at) != 0)) ++bad;
                free(out);
            }
            free(s);
        }
    return bad;
}

struct Image {
    JpegScan s;
    int n_seg, ri, per, n_bytes;
    const int32_t* segs;
    const uint8_t* stream;
};

// -> status; *n_sub, *rounds, *walks as the sync kernel counts them
static int run_split(const Image& im, int S, int* n_sub, int* rounds, int* walks) {
    int status = 0;
    jpeg_segment_mcus(im.n_seg, im.ri, im.s.total_mcus, &status);        // the image-level check of the sync kernel
    // de-stuff: each segment alone in a block of its own size, the copy in a block of its de-stuffed length + 8
    std::vector<uint8_t*> copies(im.n_seg);
    std::vector<int> dlen(im.n_seg);
    for (int k = 0; k < im.n_seg; ++k) {
        const int begin = im.segs[k], n = jpeg_segment_end(im.segs, k, im.n_seg, im.n_bytes) - begin;
        uint8_t* one = static_cast<uint8_t*>(malloc(n ? n : 1));
        memcpy(one, im.stream + begin, n);
        const int total = jpeg_destuff_range(one, 0, n, nullptr);
        uint8_t* dst = static_cast<uint8_t*>(malloc(total + 8));
        memset(dst + total, 0, 8);
        int base = 0;
        for (int t0 = 0; t0 < n; t0 += 1024) {
            int cnt[64], sum = 0;
            for (int lane = 0; lane < 64; ++lane) {
                const int lo = t0 + lane * 16, hi = lo + 16 < n ? lo + 16 : n;
                cnt[lane] = lo < hi ? jpeg_destuff_range(one, lo, hi, nullptr) : 0;
            }
            for (int lane = 0; lane < 64; ++lane) {
                const int lo = t0 + lane * 16, hi = lo + 16 < n ? lo + 16 : n;
                if (lo < hi) jpeg_destuff_range(one, lo, hi, dst + base + sum);
                sum += cnt[lane];
            }
            base += sum;
        }
        if (base != total) { fprintf(stderr, "de-stuffed length %d != %d\n", base, total); exit(1); }
        free(one);
        copies[k] = dst;
        dlen[k] = total;
    }
    const int n_slots = im.n_bytes / S + im.n_seg + 1;
    JpegSubRec* recs = static_cast<JpegSubRec*>(malloc(sizeof(JpegSubRec) * n_slots));
    *n_sub = *rounds = *walks = 0;
    for (int i = 0; i < n_slots; ++i) {                              // round 0
        const int k = jpeg_split_slot_segment(im.segs, im.n_seg, i, S);
        const int j = i - jpeg_split_slot_base(im.segs[k], k, S);
        const bool on = j >= 0 && j < jpeg_subseq_count(dlen[k], S);
        JpegSubRec r;
        memset(&r, 0, sizeof r);
        r.entry = on && j > 0 ? jpeg_sync_pack(jpeg_sync_guess(j, S)) : 0;
        r.seg = k;
        r.j = on ? j : -1;
        if (on) {
            jpeg_split_walk_item(r, copies[k], dlen[k], S, im.s);
            ++*walks;
            ++*n_sub;
        }
        recs[i] = r;
    }
    for (;;) {
        bool changed = false;
        for (int i = n_slots - 1; i >= 0; --i)                       // entries from the exits of the round before
            if (recs[i].j > 0 && jpeg_split_repair_item(recs[i], recs[i - 1].exit, S)) changed = true;
        if (!changed || *rounds >= n_slots) break;
        ++*rounds;
        for (int i = 0; i < n_slots; ++i) {
            if (recs[i].j < 0 || !recs[i].dirty) continue;
            jpeg_split_walk_item(recs[i], copies[recs[i].seg], dlen[recs[i].seg], S, im.s);
            ++*walks;
        }
    }
    uint32_t run[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < n_slots; ++i) {                              // exclusive scan per segment
        JpegSubRec& r = recs[i];
        if (r.j <= 0) run[0] = run[1] = run[2] = run[3] = run[4] = 0;
        r.pre_blocks = (int32_t)run[0];
        r.pre_dc[0] = run[1]; r.pre_dc[1] = run[2]; r.pre_dc[2] = run[3];
        r.pre_bad = (int32_t)run[4];
        run[0] += (uint32_t)r.blocks; run[1] += r.dc[0]; run[2] += r.dc[1]; run[3] += r.dc[2];
        run[4] += r.j >= 0 && ((r.exit >> 48) & 255) != 0 ? 1u : 0u;
    }
    for (int i = n_slots - 1; i >= 0; --i) {                         // write pass, in any order
        if (recs[i].j < 0) continue;
        const int k = recs[i].seg;
        status |= jpeg_split_write_item(recs[i], copies[k], dlen[k], jpeg_subseq_count(dlen[k], S), S, im.per, im.s);
    }
    free(recs);
    for (uint8_t* c : copies) free(c);
    return status;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin 8,32,128\n", argv[0]); return 2; }
    std::vector<int> sizes;
    for (const char* p = argv[2]; *p;) {
        char* e;
        const long v = strtol(p, &e, 10);
        if (e == p || v < 8 || v > 4096 || v % 4) { fprintf(stderr, "bad subsequence size\n"); return 2; }
        sizes.push_back((int)v);
        p = *e == ',' ? e + 1 : e;
    }
    const int ds = destuff_self_test();
    if (ds) { fprintf(stderr, "de-stuffing rule: %d mismatches\n", ds); return 1; }
    printf("DESTUFF OK\n");
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
        for (int k = 0; k < nseg; ++k) {
            const int end = jpeg_segment_end(segs, k, nseg, nbytes);
            if (segs[k] < 0 || end < segs[k] || end > nbytes) { fprintf(stderr, "case %d: segment table\n", ci); return 2; }
        }
        uint8_t* zigzag = static_cast<uint8_t*>(malloc(64));
        for (int k = 0; k < 64; ++k) zigzag[k] = (uint8_t)jpeg_zigzag(k);
        Image im;
        JpegScan& s = im.s;
        s.zigzag = zigzag;
        s.n_components = nc; s.h_samp = hs; s.v_samp = vs;
        s.mcus_w = (width + 8 * hs - 1) / (8 * hs);
        const int mcus_h = (height + 8 * vs - 1) / (8 * vs);
        s.total_mcus = s.mcus_w * mcus_h;
        size_t blocks[3] = {0, 0, 0}, total_blocks = 0;
        for (int c = 0; c < 3; ++c) { s.blocks_w[c] = 0; s.coef[c] = nullptr; s.dc[c] = s.ac[c] = &tabs[0]; }
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
        std::vector<int16_t> want;
        if (expect == 0) {
            want.resize(total_blocks * 64);
            if (!rd(f, want.data(), want.size() * sizeof(int16_t))) return 2;
        }
        const size_t coef_bytes = total_blocks * 64 * sizeof(int16_t);
        auto planes = [&](int16_t* coef) { size_t at = 0; for (int c = 0; c < nc; ++c) { s.coef[c] = coef + at * 64; at += blocks[c]; } };

        // the lane-per-segment decoder on the same stream
        int16_t* seq = static_cast<int16_t*>(calloc(total_blocks * 64, sizeof(int16_t)));
        planes(seq);
        int seq_status = 0;
        const int per = jpeg_segment_mcus(nseg, ri, s.total_mcus, &seq_status);
        for (int k = 0; k < nseg; ++k) {
            const int end = jpeg_segment_end(segs, k, nseg, nbytes);
            uint8_t* one = static_cast<uint8_t*>(malloc(end - segs[k] ? end - segs[k] : 1));
            memcpy(one, stream + segs[k], end - segs[k]);
            seq_status |= jpeg_decode_segment(one, end - segs[k], k * per, per, s);
            free(one);
        }
        if (expect == 0 && (seq_status != 0 || memcmp(want.data(), seq, coef_bytes) != 0)) {
            fprintf(stderr, "case %d: the sequential decoder misses the file's coefficients\n", ci);
            ++failures;
        }
        if (expect != 0 && seq_status == 0) { fprintf(stderr, "case %d: status 0 on a corrupt stream\n", ci); ++failures; }

        im.n_seg = nseg; im.ri = ri; im.per = per; im.n_bytes = nbytes; im.segs = segs; im.stream = stream;
        for (int S : sizes) {
            int16_t* coef = static_cast<int16_t*>(calloc(total_blocks * 64, sizeof(int16_t)));
            planes(coef);
            int n_sub, rounds, walks;
            const int status = run_split(im, S, &n_sub, &rounds, &walks);
            printf("%d %d %d %d %d %d\n", ci, S, status, n_sub, rounds, walks);
            if (status != seq_status) { fprintf(stderr, "case %d at %d: status %d, sequential %d\n", ci, S, status, seq_status); ++failures; }
            if (rounds > n_sub) { fprintf(stderr, "case %d at %d: %d rounds for %d subsequences\n", ci, S, rounds, n_sub); ++failures; }
            if (expect == 0 && (memcmp(want.data(), coef, coef_bytes) != 0 || memcmp(seq, coef, coef_bytes) != 0)) {
                fprintf(stderr, "case %d at %d: coefficients differ\n", ci, S);
                ++failures;
            }
            free(coef);
        }
        free(seq); free(stream); free(segs); free(tabs); free(zigzag);
    }
    fclose(f);
    if (failures) { fprintf(stderr, "%d requirement(s) failed\n", failures); return 1; }
    printf("OK %d cases\n", head[1]);
    return 0;
}
