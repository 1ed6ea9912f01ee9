// Stand-alone host build of the motion-compensated GOP path of csrc/sdv_h264_core.h (test_h264_me_cpu.py compiles it with
// -fsanitize=address,undefined and runs it): the fetch-address function and the macroblock step with a vector, the same functions the
// kernel runs, over a whole call, on buffers of exactly the planes' size - a fetch outside them is a sanitizer report.  The vectors are
// given, not searched: valid, extreme and invalid ones alike go through h264_mv_fetch.
//   h264_me_host_main IN OUT
// IN : int32 n, mbh, mbw, qp, gop, first_index, search; y [n][16 mbh][16 mbw]; cb, cr [n][8 mbh][8 mbw]; int16 mv [n][mbh][mbw][2]
// OUT: per picture int32 length and the sample; the reconstruction planes in the layout of the input; int16 the vectors that were coded
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sdv_h264_core.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t hd[7];
    if (fread(hd, 4, 7, in) != 7) return 2;
    const int n = hd[0], mbh = hd[1], mbw = hd[2], qp = hd[3], gop = hd[4], first_index = hd[5], search = hd[6];
    const size_t ly = (size_t)n * mbh * 16 * mbw * 16, lc = ly / 4, lm = (size_t)n * mbh * mbw * 2;
    std::vector<uint8_t> y(ly), cb(lc), cr(lc), ry(ly), rcb(lc), rcr(lc);
    std::vector<int16_t> mv(lm), used(lm, 0);
    if (fread(y.data(), 1, ly, in) != ly || fread(cb.data(), 1, lc, in) != lc || fread(cr.data(), 1, lc, in) != lc) return 2;
    if (fread(mv.data(), 2, lm, in) != lm) return 2;
    fclose(in);
    const int slot_mbw = mbw + 1 + mbw / 64;
    const long long slot = 600LL * slot_mbw + 17;                                  // the capacity of one slice, exactly
    const long long lw = 16LL * mbw, cw = 8LL * mbw;
    std::vector<std::vector<uint8_t>> slots((size_t)n * mbh, std::vector<uint8_t>((size_t)slot));
    std::vector<long long> lens((size_t)n * mbh);
    h264_gop_mb* mb = new h264_gop_mb;
    for (int k = 0; k < gop && k < n; ++k)                                         // one picture position after the other, as the launches
        for (int g = 0; g * gop + k < n; ++g)
            for (int r = 0; r < mbh; ++r) {
                const long long f = (long long)g * gop + k, row = f * mbh + r;
                const bool p = k > 0;
                uint8_t* s = slots[(size_t)row].data();
                h264_writer w;
                h264_chain ch;
                h264_mv_chain mvc;
                int skip_run = 0;
                w.init(s + 5, slot - 5);
                ch.have = 0;
                mvc.vx = mvc.vy = 0;
                if (p) h264_p_slice_header(w, (unsigned)(r * mbw), (unsigned)k, qp);
                else h264_slice_header(w, (unsigned)(r * mbw), (unsigned)((first_index + f) & 1), qp);
                const long long yat = row * 16 * lw, cat = row * 8 * cw;
                for (int m = 0; m < mbw; ++m) {
                    h264_mv_ref at;
                    at.vx = at.vy = 0;
                    for (int i = 0; i < 16; ++i) memcpy(mb->sy + i * 16, y.data() + yat + i * lw + m * 16, 16);
                    for (int c = 0; c < 2; ++c)
                        for (int i = 0; i < 8; ++i) memcpy(mb->sc + c * 64 + i * 8, (c ? cr : cb).data() + cat + i * cw + m * 8, 8);
                    if (p) {
                        const int16_t* v = mv.data() + ((size_t)row * mbw + m) * 2;
                        at = h264_mv_fetch(v[0], v[1], search, m, r, mbw, mbh);
                        if (!h264_mv_valid(at.vx, at.vy, search, m, r, mbw, mbh)) return 4;
                        const uint8_t* py = ry.data() + (f - 1) * mbh * 16 * lw + at.yoff;      // picture f - 1, displaced
                        for (int i = 0; i < 16; ++i) memcpy(mb->fy + i * 16, py + i * lw, 16);
                        for (int c = 0; c < 2; ++c) {
                            const uint8_t* pc = (c ? rcr : rcb).data() + (f - 1) * mbh * 8 * cw + at.coff;
                            for (int i = 0; i < 8; ++i) memcpy(mb->fc + c * 64 + i * 8, pc + i * cw, 8);
                        }
                        used[((size_t)row * mbw + m) * 2] = (int16_t)at.vx, used[((size_t)row * mbw + m) * 2 + 1] = (int16_t)at.vy;
                    }
                    h264_gop_encode_mb_mv(mb, ch, mvc, p, qp, at.vx, at.vy, w, &skip_run);
                    for (int i = 0; i < 16; ++i) memcpy(ry.data() + yat + i * lw + m * 16, mb->ry + i * 16, 16);
                    for (int c = 0; c < 2; ++c)
                        for (int i = 0; i < 8; ++i) memcpy((c ? rcr : rcb).data() + cat + i * cw + m * 8, mb->rc + c * 64 + i * 8, 8);
                }
                if (p && skip_run) h264_put_ue(w, (unsigned)skip_run);
                w.put(1u, 1);
                while (w.n) w.put(0u, 1);
                if (w.pos > slot - 5) return 3;                                    // the capacity bound was broken
                const unsigned len = (unsigned)(1 + w.pos);
                s[0] = (uint8_t)(len >> 24), s[1] = (uint8_t)(len >> 16), s[2] = (uint8_t)(len >> 8), s[3] = (uint8_t)len;
                s[4] = p ? 0x41 : 0x65;
                lens[(size_t)row] = 5 + w.pos;
            }
    delete mb;
    // the search's order as one word: unpacking gives back what was packed, and the word orders as the tuple does
    for (int vy = -kH264SearchMax; vy <= kH264SearchMax; vy += 2)
        for (int vx = -kH264SearchMax; vx <= kH264SearchMax; vx += 2) {
            int cost, ax, ay;
            h264_me_unkey(h264_me_key(h264_me_cost(65280, h264_me_lambda(51), vx, vy), vx, vy), &cost, &ax, &ay);
            if (ax != vx || ay != vy || cost != h264_me_cost(65280, h264_me_lambda(51), vx, vy) || cost >= (1 << 17)) return 5;
        }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    for (int f = 0; f < n; ++f) {
        int32_t total = 0;
        for (int r = 0; r < mbh; ++r) total += (int32_t)lens[(size_t)f * mbh + r];
        fwrite(&total, 4, 1, out);
        for (int r = 0; r < mbh; ++r) fwrite(slots[(size_t)f * mbh + r].data(), 1, (size_t)lens[(size_t)f * mbh + r], out);
    }
    fwrite(ry.data(), 1, ly, out), fwrite(rcb.data(), 1, lc, out), fwrite(rcr.data(), 1, lc, out);
    fwrite(used.data(), 2, lm, out);
    fclose(out);
    return 0;
}
