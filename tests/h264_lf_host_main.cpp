// Stand-alone host build of the loop filter pieces of csrc/sdv_h264_core.h (test_h264_lf_cpu.py compiles it with
// -fsanitize=address,undefined and runs it): the slice headers with the filter on, the side information word of every macroblock
// (h264_lf_word), and h264_lf_picture - bS, index, the one line filter - between two picture positions, around the macroblock steps the
// kernels run (h264_i4_encode_mb, h264_gop_encode_mb_mv, h264_gop_encode_mb_sub), on heap buffers of exactly the planes', the slots', the
// vectors' and the words' sizes: a read outside a plane or a store beyond a buffer is a sanitizer report.
//   h264_lf_host_main IN OUT
// IN : int32 n, mbh, mbw, qp, gop, first_index, search (0 = zero vectors), subpel (0 = even whole samples in mv), intra4;
//      y [n][16 mbh][16 mbw]; cb, cr [n][8 mbh][8 mbw]; mv int16 [n][mbh][mbw][2]
// OUT: per picture int32 length and the sample; the FILTERED reconstruction planes in the layout of the input; the words uint32
//      [n][mbh][mbw]; then the tables: alpha [52], beta [52], tc0 [52][3] as bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sdv_h264_core.h"

namespace {
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
    int32_t hd[9];
    if (fread(hd, 4, 9, in) != 9) return 2;
    const int n = hd[0], mbh = hd[1], mbw = hd[2], qp = hd[3], gop = hd[4], first_index = hd[5], search = hd[6], subpel = hd[7], intra4 = hd[8];
    if (subpel && !h264_subpel_ok(subpel)) return 2;
    const size_t ly = (size_t)n * mbh * 16 * mbw * 16, lc = ly / 4, lm = (size_t)n * mbh * mbw * 2;
    std::vector<uint8_t> y(ly), cb(lc), cr(lc), ry(ly), rcb(lc), rcr(lc);
    std::vector<int16_t> mv(lm);
    std::vector<uint32_t> words(lm / 2, 0xffffffffu);
    if (fread(y.data(), 1, ly, in) != ly || fread(cb.data(), 1, lc, in) != lc || fread(cr.data(), 1, lc, in) != lc) return 2;
    if (fread(mv.data(), 2, lm, in) != lm) return 2;
    fclose(in);
    const int slot_mbw = mbw + 1 + mbw / 64;
    const long long slot = 600LL * slot_mbw + 17;                                  // the capacity of one slice, exactly
    const long long lw = 16LL * mbw, cw = 8LL * mbw;
    const size_t pic_y = (size_t)mbh * 16 * lw, pic_c = (size_t)mbh * 8 * cw, pic_mb = (size_t)mbh * mbw;
    std::vector<std::vector<uint8_t>> slots((size_t)n * mbh, std::vector<uint8_t>((size_t)slot));
    std::vector<long long> lens((size_t)n * mbh);
    std::vector<uint8_t> wy((size_t)kH264SubLumaWin * kH264SubLumaWin), wc((size_t)2 * kH264SubChromaWin * kH264SubChromaWin);
    h264_gop_mb* mb = new h264_gop_mb;
    h264_i4_mb* i4 = new h264_i4_mb;
    const int range = search ? search : 2;
    for (int k = 0; k < gop && k < n; ++k) {                                       // one picture position after the other, as the launches
        for (int g = 0; g * gop + k < n; ++g)
            for (int r = 0; r < mbh; ++r) {
                const long long f = (long long)g * gop + k, row = f * mbh + r;
                const bool p = k > 0;
                uint8_t* s = slots[(size_t)row].data();
                h264_writer w;
                h264_i4_chain ch;
                h264_mv_chain mvc;
                int skip_run = 0;
                w.init(s + 5, slot - 5);
                ch.ch.have = 0;
                mvc.vx = mvc.vy = 0;
                if (p) h264_p_slice_header(w, (unsigned)(r * mbw), (unsigned)k, qp, 1);
                else h264_slice_header(w, (unsigned)(r * mbw), (unsigned)((first_index + f) & 1), qp, 1);
                const long long yat = row * 16 * lw, cat = row * 8 * cw;
                for (int m = 0; m < mbw; ++m) {
                    for (int i = 0; i < 16; ++i) memcpy(mb->sy + i * 16, y.data() + yat + i * lw + m * 16, 16);
                    for (int c = 0; c < 2; ++c)
                        for (int i = 0; i < 8; ++i) memcpy(mb->sc + c * 64 + i * 8, (c ? cr : cb).data() + cat + i * cw + m * 8, 8);
                    const int16_t* v = mv.data() + ((size_t)row * mbw + m) * 2;
                    int vx = 0, vy = 0;
                    unsigned nz = 0;
                    if (!p && intra4) {
                        h264_i4_encode_mb(mb, i4, ch, qp, w);
                    } else if (subpel) {
                        h264_sub_ref at = h264_sub_fetch(0, 0, range, subpel, m, r, mbw, mbh);
                        if (p) {
                            at = h264_sub_fetch(v[0], v[1], range, subpel, m, r, mbw, mbh);
                            stage(at, ry.data() + (size_t)(f - 1) * pic_y, rcb.data() + (size_t)(f - 1) * pic_c, rcr.data() + (size_t)(f - 1) * pic_c, m, r,
                                  mbw, mbh, wy, wc);
                        }
                        h264_gop_encode_mb_sub(mb, ch.ch, mvc, p, qp, at, wy.data(), wc.data(), w, &skip_run);
                        vx = at.vx, vy = at.vy;
                    } else {
                        h264_mv_ref at = h264_mv_fetch(0, 0, range, m, r, mbw, mbh);
                        if (p) {
                            at = h264_mv_fetch(v[0], v[1], range, m, r, mbw, mbh);
                            const uint8_t* fy = ry.data() + (size_t)(f - 1) * pic_y + at.yoff;
                            for (int i = 0; i < 16; ++i) memcpy(mb->fy + i * 16, fy + i * lw, 16);
                            for (int c = 0; c < 2; ++c)
                                for (int i = 0; i < 8; ++i)
                                    memcpy(mb->fc + c * 64 + i * 8, (c ? rcr : rcb).data() + (size_t)(f - 1) * pic_c + at.coff + i * cw, 8);
                        }
                        h264_gop_encode_mb_mv(mb, ch.ch, mvc, p, qp, at.vx, at.vy, w, &skip_run);
                        vx = at.vx, vy = at.vy;
                    }
                    if (mb->mode == kH264ModeInter)                                 // what the kernel's ballot holds: the blocks with a nonzero level
                        for (int b = 0; b < 16; ++b)
                            for (int i = 0; i < 16; ++i)
                                if (mb->lev[(1 + b) * 16 + i]) nz |= 1u << b;
                    words[(size_t)row * mbw + m] = h264_lf_word(mb->mode, nz, vx, vy);
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
        for (int g = 0; g * gop + k < n; ++g) {                                    // the filter launch of position k
            const size_t f = (size_t)g * gop + k;
            h264_lf_picture(ry.data() + f * pic_y, rcb.data() + f * pic_c, rcr.data() + f * pic_c, mbh, mbw, qp, words.data() + f * pic_mb,
                            mv.data() + f * pic_mb * 2, subpel);
        }
    }
    delete mb;
    delete i4;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    for (int f = 0; f < n; ++f) {
        int32_t total = 0;
        for (int r = 0; r < mbh; ++r) total += (int32_t)lens[(size_t)f * mbh + r];
        fwrite(&total, 4, 1, out);
        for (int r = 0; r < mbh; ++r) fwrite(slots[(size_t)f * mbh + r].data(), 1, (size_t)lens[(size_t)f * mbh + r], out);
    }
    fwrite(ry.data(), 1, ly, out), fwrite(rcb.data(), 1, lc, out), fwrite(rcr.data(), 1, lc, out);
    fwrite(words.data(), 4, words.size(), out);
    uint8_t tables[52 * 5];
    for (int i = 0; i < 52; ++i) {
        tables[i] = (uint8_t)h264_lf_alpha(i), tables[52 + i] = (uint8_t)h264_lf_beta(i);
        for (int b = 1; b <= 3; ++b) tables[104 + 3 * i + b - 1] = (uint8_t)h264_lf_tc0(i, b);
    }
    fwrite(tables, 1, sizeof tables, out);
    fclose(out);
    return 0;
}
