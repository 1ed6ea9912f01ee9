// Stand-alone host build of the Intra4x4 pieces of csrc/sdv_h264_core.h (test_h264_i4_cpu.py compiles it with
// -fsanitize=address,undefined and runs it): h264_i4_encode_mb - edges, the one predictor, the block chain, the I_NxN coder, the
// Intra16x16 and I_PCM ways out - the same functions the kernel runs, over a call of IDR pictures, on heap buffers of exactly the planes'
// and the slots' sizes: a read outside the macroblock state or a store beyond a slot is a sanitizer report.
//   h264_i4_host_main IN OUT
// IN : int32 n, mbh, mbw, qp, first_index; y [n][16 mbh][16 mbw]; cb, cr [n][8 mbh][8 mbw]
// OUT: per picture int32 length and the sample; the reconstruction planes in the layout of the input; per macroblock one byte, its
//      h264_gop_mb::mode; then, for the first 13 samples of every picture's luma as an edge vector (corner, top 0 .. 7, left 0 .. 3) with
//      everything available, the nine predictions [mode][y][x]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sdv_h264_core.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t hd[5];
    if (fread(hd, 4, 5, in) != 5) return 2;
    const int n = hd[0], mbh = hd[1], mbw = hd[2], qp = hd[3], first_index = hd[4];
    const size_t ly = (size_t)n * mbh * 16 * mbw * 16, lc = ly / 4;
    std::vector<uint8_t> y(ly), cb(lc), cr(lc), ry(ly), rcb(lc), rcr(lc), kinds((size_t)n * mbh * mbw);
    if (fread(y.data(), 1, ly, in) != ly || fread(cb.data(), 1, lc, in) != lc || fread(cr.data(), 1, lc, in) != lc) return 2;
    fclose(in);
    const int slot_mbw = mbw + 1 + mbw / 64;
    const long long slot = 600LL * slot_mbw + 17;                                  // the capacity of one slice, exactly
    const long long lw = 16LL * mbw, cw = 8LL * mbw;
    std::vector<std::vector<uint8_t>> slots((size_t)n * mbh, std::vector<uint8_t>((size_t)slot));
    std::vector<long long> lens((size_t)n * mbh);
    h264_gop_mb* mb = new h264_gop_mb;
    h264_i4_mb* i4 = new h264_i4_mb;
    for (int f = 0; f < n; ++f)
        for (int r = 0; r < mbh; ++r) {
            const long long row = (long long)f * mbh + r;
            uint8_t* s = slots[(size_t)row].data();
            h264_writer w;
            h264_i4_chain ch;
            w.init(s + 5, slot - 5);
            ch.ch.have = 0;
            h264_slice_header(w, (unsigned)(r * mbw), (unsigned)((first_index + f) & 1), qp);
            const long long yat = row * 16 * lw, cat = row * 8 * cw;
            for (int m = 0; m < mbw; ++m) {
                for (int i = 0; i < 16; ++i) memcpy(mb->sy + i * 16, y.data() + yat + i * lw + m * 16, 16);
                for (int c = 0; c < 2; ++c)
                    for (int i = 0; i < 8; ++i) memcpy(mb->sc + c * 64 + i * 8, (c ? cr : cb).data() + cat + i * cw + m * 8, 8);
                kinds[(size_t)row * mbw + m] = (uint8_t)h264_i4_encode_mb(mb, i4, ch, qp, w);
                for (int i = 0; i < 16; ++i) memcpy(ry.data() + yat + i * lw + m * 16, mb->ry + i * 16, 16);
                for (int c = 0; c < 2; ++c)
                    for (int i = 0; i < 8; ++i) memcpy((c ? rcr : rcb).data() + cat + i * cw + m * 8, mb->rc + c * 64 + i * 8, 8);
            }
            w.put(1u, 1);
            while (w.n) w.put(0u, 1);
            if (w.pos > slot - 5) return 3;                                        // the capacity bound was broken
            const unsigned len = (unsigned)(1 + w.pos);
            s[0] = (uint8_t)(len >> 24), s[1] = (uint8_t)(len >> 16), s[2] = (uint8_t)(len >> 8), s[3] = (uint8_t)len;
            s[4] = 0x65;
            lens[(size_t)row] = 5 + w.pos;
        }
    delete mb;
    delete i4;
    for (int cbp = 0; cbp < 48; ++cbp)                                             // the intra column is a permutation
        for (int other = 0; other < cbp; ++other)
            if (h264_cbp_intra_code(cbp) == h264_cbp_intra_code(other) || h264_cbp_intra_code(cbp) > 47) return 5;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    for (int f = 0; f < n; ++f) {
        int32_t total = 0;
        for (int r = 0; r < mbh; ++r) total += (int32_t)lens[(size_t)f * mbh + r];
        fwrite(&total, 4, 1, out);
        for (int r = 0; r < mbh; ++r) fwrite(slots[(size_t)f * mbh + r].data(), 1, (size_t)lens[(size_t)f * mbh + r], out);
    }
    fwrite(ry.data(), 1, ly, out), fwrite(rcb.data(), 1, lc, out), fwrite(rcr.data(), 1, lc, out);
    fwrite(kinds.data(), 1, kinds.size(), out);
    for (int f = 0; f < n; ++f) {
        std::vector<uint8_t> edge(y.begin() + (long long)f * mbh * 16 * lw, y.begin() + (long long)f * mbh * 16 * lw + 13);
        uint8_t pred[kH264I4Modes * 16];
        for (int mode = 0; mode < kH264I4Modes; ++mode)
            for (int i = 0; i < 16; ++i)
                pred[mode * 16 + i] = (uint8_t)h264_i4_pred(edge.data(), kH264I4Top | kH264I4Left | kH264I4Corner | kH264I4TopRight, mode, i & 3, i >> 2);
        fwrite(pred, 1, sizeof pred, out);
    }
    fclose(out);
    return 0;
}
