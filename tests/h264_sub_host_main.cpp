// Stand-alone host build of the sub-sample motion pieces of csrc/sdv_h264_core.h (test_h264_sub_cpu.py compiles it with
// -fsanitize=address,undefined and runs it): h264_sub_fetch, the clamped window addresses, the two interpolators and the macroblock step
// with a quarter-sample vector - the same functions the kernels run - over a whole call, on heap buffers of exactly the planes' and the
// windows' sizes: a fetch or a tap outside them is a sanitizer report.  The vectors are given, not searched: valid, extreme and invalid
// ones alike go through h264_sub_fetch.
//   h264_sub_host_main IN OUT
// IN : int32 n, mbh, mbw, qp, gop, first_index, search, subpel; y [n][16 mbh][16 mbw]; cb, cr [n][8 mbh][8 mbw]; int16 mv [n][mbh][mbw][2]
// OUT: per picture int32 length and the sample; the reconstruction planes in the layout of the input; int16 the vectors that were coded;
//      then, from source picture 0, for each corner macroblock (top left, top right, bottom left, bottom right) and each of the 16
//      fractions (yf * 4 + xf) the 256 luma and 64 Cb samples predicted by the vector with that fraction whose whole part points inward
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sdv_h264_core.h"

namespace {
// the two windows of macroblock (m, r) for ``at``, on the heap at exactly their sizes
void stage(const h264_sub_ref& at, const uint8_t* py, const uint8_t* pcb, const uint8_t* pcr, int m, int r, int mbw, int mbh, std::vector<uint8_t>& wy,
           std::vector<uint8_t>& wc) {
    const int nl = kH264SubLumaWin * kH264SubLumaWin, nc = kH264SubChromaWin * kH264SubChromaWin;
    for (int i = 0; i < nl; ++i) wy[(size_t)i] = py[h264_sub_luma_at(at, i, m, r, mbw, mbh)];
    for (int i = 0; i < nc; ++i) {
        const long long from = h264_sub_chroma_at(at, i, m, r, mbw, mbh);
        wc[(size_t)i] = pcb[from], wc[(size_t)(nc + i)] = pcr[from];
    }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t hd[8];
    if (fread(hd, 4, 8, in) != 8) return 2;
    const int n = hd[0], mbh = hd[1], mbw = hd[2], qp = hd[3], gop = hd[4], first_index = hd[5], search = hd[6], subpel = hd[7];
    if (!h264_subpel_ok(subpel)) return 2;
    const size_t ly = (size_t)n * mbh * 16 * mbw * 16, lc = ly / 4, lm = (size_t)n * mbh * mbw * 2;
    std::vector<uint8_t> y(ly), cb(lc), cr(lc), ry(ly), rcb(lc), rcr(lc);
    std::vector<int16_t> mv(lm), used(lm, 0);
    if (fread(y.data(), 1, ly, in) != ly || fread(cb.data(), 1, lc, in) != lc || fread(cr.data(), 1, lc, in) != lc) return 2;
    if (fread(mv.data(), 2, lm, in) != lm) return 2;
    fclose(in);
    const int slot_mbw = mbw + 1 + mbw / 64;
    const long long slot = 600LL * slot_mbw + 17;                                  // the capacity of one slice, exactly
    const long long lw = 16LL * mbw, cw = 8LL * mbw;
    const size_t pic_y = (size_t)mbh * 16 * lw, pic_c = (size_t)mbh * 8 * cw;
    std::vector<std::vector<uint8_t>> slots((size_t)n * mbh, std::vector<uint8_t>((size_t)slot));
    std::vector<long long> lens((size_t)n * mbh);
    std::vector<uint8_t> wy((size_t)kH264SubLumaWin * kH264SubLumaWin), wc((size_t)2 * kH264SubChromaWin * kH264SubChromaWin);
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
                    h264_sub_ref at = h264_sub_fetch(0, 0, search, subpel, m, r, mbw, mbh);
                    for (int i = 0; i < 16; ++i) memcpy(mb->sy + i * 16, y.data() + yat + i * lw + m * 16, 16);
                    for (int c = 0; c < 2; ++c)
                        for (int i = 0; i < 8; ++i) memcpy(mb->sc + c * 64 + i * 8, (c ? cr : cb).data() + cat + i * cw + m * 8, 8);
                    if (p) {
                        const int16_t* v = mv.data() + ((size_t)row * mbw + m) * 2;
                        at = h264_sub_fetch(v[0], v[1], search, subpel, m, r, mbw, mbh);
                        if (!h264_sub_valid(at.vx, at.vy, search, subpel, m, r, mbw, mbh)) return 4;
                        stage(at, ry.data() + (size_t)(f - 1) * pic_y, rcb.data() + (size_t)(f - 1) * pic_c, rcr.data() + (size_t)(f - 1) * pic_c, m, r,
                              mbw, mbh, wy, wc);
                        used[((size_t)row * mbw + m) * 2] = (int16_t)at.vx, used[((size_t)row * mbw + m) * 2 + 1] = (int16_t)at.vy;
                    }
                    h264_gop_encode_mb_sub(mb, ch, mvc, p, qp, at, wy.data(), wc.data(), w, &skip_run);
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
    unsigned long long before = 0;
    for (int cost = 0; cost <= 70000; cost += 70000)
        for (int a = 0; a <= 128; ++a)                                             // ascending (|vx| + |vy|, vy, vx) at one cost
            for (int vy = -64; vy <= 64; ++vy)
                for (int vx = -64; vx <= 64; ++vx) {
                    if ((vx < 0 ? -vx : vx) + (vy < 0 ? -vy : vy) != a) continue;
                    const unsigned long long key = h264_sub_key(cost, vx, vy);
                    int c2, ax, ay;
                    h264_sub_unkey(key, &c2, &ax, &ay);
                    if (ax != vx || ay != vy || c2 != cost || (before && key <= before)) return 5;
                    before = key;
                }
    if (h264_sub_cost(65280, h264_me_lambda(51), 64, -64) >= 70000) return 5;
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
    // all 16 positions at all four corners, from source picture 0 (quarter grid, whatever the call's subpel)
    for (int corner = 0; corner < 4; ++corner)
        for (int fr = 0; fr < 16; ++fr) {
            const int m = (corner & 1) ? mbw - 1 : 0, r = (corner & 2) ? mbh - 1 : 0, xf = fr & 3, yf = fr >> 2;
            const int vx = xf - ((corner & 1) && xf ? 4 : 0), vy = yf - ((corner & 2) && yf ? 4 : 0);
            const h264_sub_ref at = h264_sub_fetch(vx, vy, 2, 4, m, r, mbw, mbh);  // (a one-macroblock-wide picture admits no fraction: (0, 0))
            stage(at, y.data(), cb.data(), cr.data(), m, r, mbw, mbh, wy, wc);
            uint8_t py[256], pc[64];
            for (int i = 0; i < 256; ++i) py[i] = (uint8_t)h264_sub_pred_luma(wy.data(), at, i & 15, i >> 4);
            for (int i = 0; i < 64; ++i) pc[i] = (uint8_t)h264_sub_pred_chroma(wc.data(), at, i & 7, i >> 3);
            const int16_t coded[2] = {(int16_t)at.vx, (int16_t)at.vy};
            fwrite(coded, 2, 2, out), fwrite(py, 1, 256, out), fwrite(pc, 1, 64, out);
        }
    fclose(out);
    return 0;
}
