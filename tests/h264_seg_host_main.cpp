// Stand-alone host build of the row-slice pieces of csrc/sdv_h264_core.h (test_h264_seg_cpu.py compiles it with
// -fsanitize=address,undefined and runs it): the number of slices a row gets (h264_row_segments), a slice's bounds (h264_seg_first), its
// slot index and the seg layout, around the four-vector macroblock coder (h264_gop_encode_mb_part) and the Intra4x4 one
// (h264_i4_encode_mb) started afresh at every slice, and the four-vector loop filter over whole pictures - on heap buffers of exactly the
// planes', the slots', the vectors' and the words' sizes: a read outside a plane or a store beyond a slot is a sanitizer report.
//   h264_seg_host_main IN OUT
// IN : int32 n, mbh, mbw, qp, gop, first_index, search (>= 2), subpel (0, 1, 2, 4), intra4, deblock, row_slices;
//      y [n][16 mbh][16 mbw]; cb, cr [n][8 mbh][8 mbw]; mv int16 [n][mbh][mbw][4][2]
// OUT: int32 segs; per picture int32 length and the sample (its mbh segs slices in slot order); the reconstruction planes (filtered with
//      deblock) in the layout of the input; the words uint32 [n][mbh][mbw]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sdv_h264_core.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t hd[11];
    if (fread(hd, 4, 11, in) != 11) return 2;
    const int n = hd[0], mbh = hd[1], mbw = hd[2], qp = hd[3], gop = hd[4], first_index = hd[5], search = hd[6], subpel = hd[7], intra4 = hd[8],
              deblock = hd[9], row_slices = hd[10];
    if (!h264_part_subpel_ok(subpel) || row_slices < 1 || row_slices > kH264SegMax) return 2;
    const int segs = h264_row_segments(mbh, mbw, row_slices);
    if (!h264_seg_ok(mbh, mbw, segs)) return 2;
    const size_t ly = (size_t)n * mbh * 16 * mbw * 16, lc = ly / 4, lm = (size_t)n * mbh * mbw * 8;
    std::vector<uint8_t> y(ly), cb(lc), cr(lc), ry(ly), rcb(lc), rcr(lc);
    std::vector<int16_t> mv(lm);
    std::vector<uint32_t> words(lm / 8, 0xffffffffu);
    if (fread(y.data(), 1, ly, in) != ly || fread(cb.data(), 1, lc, in) != lc || fread(cr.data(), 1, lc, in) != lc) return 2;
    if (fread(mv.data(), 2, lm, in) != lm) return 2;
    fclose(in);
    const h264_seg_layout l = h264_seg_scratch_layout(n, mbh, mbw, segs);
    const long long slot = l.slot;                                                 // the capacity of one slice, exactly
    const long long lw = 16LL * mbw, cw = 8LL * mbw;
    const size_t pic_y = (size_t)mbh * 16 * lw, pic_c = (size_t)mbh * 8 * cw, pic_mb = (size_t)mbh * mbw;
    const int nl = kH264PartLumaWin * kH264PartLumaWin, nc = kH264PartChromaWin * kH264PartChromaWin;
    std::vector<std::vector<uint8_t>> slots((size_t)l.rows, std::vector<uint8_t>((size_t)slot));
    std::vector<long long> lens((size_t)l.rows, -1);
    std::vector<uint8_t> wy((size_t)4 * nl), wc((size_t)2 * 4 * nc);
    h264_gop_mb* mb = new h264_gop_mb;
    h264_i4_mb* i4 = new h264_i4_mb;
    for (int k = 0; k < gop && k < n; ++k) {                                       // one picture position after the other, as the launches
        for (int g = 0; g * gop + k < n; ++g)
            for (int r = 0; r < mbh; ++r)
                for (int sg = 0; sg < segs; ++sg) {
                    const long long f = (long long)g * gop + k, row = f * mbh + r;
                    const long long at_slot = h264_seg_slot_index(f, r, sg, mbh, segs);
                    const int m0 = h264_seg_first(sg, mbw, segs), m1 = h264_seg_first(sg + 1, mbw, segs);
                    if (m1 <= m0 || lens[(size_t)at_slot] != -1) return 4;         // an empty slice, or a slot written twice
                    const bool p = k > 0;
                    uint8_t* s = slots[(size_t)at_slot].data();
                    h264_writer w;
                    h264_i4_chain ch;
                    h264_part_chain pc;
                    int skip_run = 0;
                    w.init(s + 5, slot - 5);
                    ch.ch.have = 0;
                    pc.v[0][0] = pc.v[0][1] = pc.v[1][0] = pc.v[1][1] = 0;
                    if (p) h264_p_slice_header(w, (unsigned)(r * mbw + m0), (unsigned)k, qp, deblock);
                    else h264_slice_header(w, (unsigned)(r * mbw + m0), (unsigned)((first_index + f) & 1), qp, deblock);
                    const long long yat = row * 16 * lw, cat = row * 8 * cw;
                    for (int m = m0; m < m1; ++m) {
                        for (int i = 0; i < 16; ++i) memcpy(mb->sy + i * 16, y.data() + yat + i * lw + m * 16, 16);
                        for (int c = 0; c < 2; ++c)
                            for (int i = 0; i < 8; ++i) memcpy(mb->sc + c * 64 + i * 8, (c ? cr : cb).data() + cat + i * cw + m * 8, 8);
                        const int16_t* v = mv.data() + ((size_t)row * mbw + m) * 8;
                        if (!p && intra4) {
                            h264_i4_encode_mb(mb, i4, ch, qp, w);
                            words[(size_t)row * mbw + m] = h264_lf_word(mb->mode, 0u, 0, 0);
                        } else {
                            h264_sub_ref at[4];
                            for (int i = 0; i < 4; ++i) at[i] = h264_part_fetch(p ? v[2 * i] : 0, p ? v[2 * i + 1] : 0, search, subpel, m, r, mbw, mbh);
                            if (p) {
                                const uint8_t* py = ry.data() + (size_t)(f - 1) * pic_y;
                                const uint8_t* pcb = rcb.data() + (size_t)(f - 1) * pic_c;
                                const uint8_t* pcr = rcr.data() + (size_t)(f - 1) * pic_c;
                                for (int i = 0; i < 4; ++i) {
                                    for (int j = 0; j < nl; ++j) wy[(size_t)(i * nl + j)] = py[h264_part_luma_at(at[i], i, j, m, r, mbw, mbh)];
                                    for (int j = 0; j < nc; ++j) {
                                        const long long from = h264_part_chroma_at(at[i], i, j, m, r, mbw, mbh);
                                        wc[(size_t)(i * nc + j)] = pcb[from], wc[(size_t)((4 + i) * nc + j)] = pcr[from];
                                    }
                                }
                            }
                            words[(size_t)row * mbw + m] = h264_gop_encode_mb_part(mb, ch.ch, pc, p, qp, at, wy.data(), wc.data(), w, &skip_run);
                        }
                        for (int i = 0; i < 16; ++i) memcpy(ry.data() + yat + i * lw + m * 16, mb->ry + i * 16, 16);
                        for (int c = 0; c < 2; ++c)
                            for (int i = 0; i < 8; ++i) memcpy((c ? rcr : rcb).data() + cat + i * cw + m * 8, mb->rc + c * 64 + i * 8, 8);
                    }
                    if (p && skip_run) h264_put_ue(w, (unsigned)skip_run);
                    w.put(1u, 1);
                    while (w.n) w.put(0u, 1);
                    if (w.pos > slot - 5) return 3;                                // the capacity bound was broken
                    const unsigned len = (unsigned)(1 + w.pos);
                    s[0] = (uint8_t)(len >> 24), s[1] = (uint8_t)(len >> 16), s[2] = (uint8_t)(len >> 8), s[3] = (uint8_t)len;
                    s[4] = p ? 0x41 : 0x65;
                    lens[(size_t)at_slot] = 5 + w.pos;
                }
        if (deblock)
            for (int g = 0; g * gop + k < n; ++g) {                                // the filter launch of position k: it knows nothing of slices
                const size_t f = (size_t)g * gop + k;
                h264_part_lf_picture(ry.data() + f * pic_y, rcb.data() + f * pic_c, rcr.data() + f * pic_c, mbh, mbw, qp, words.data() + f * pic_mb,
                                     mv.data() + f * pic_mb * 8);
            }
    }
    delete mb;
    delete i4;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    const int32_t segs_out = segs;
    fwrite(&segs_out, 4, 1, out);
    const size_t per = (size_t)mbh * segs;
    for (int f = 0; f < n; ++f) {
        int32_t total = 0;
        for (size_t i = 0; i < per; ++i) total += (int32_t)lens[(size_t)f * per + i];
        fwrite(&total, 4, 1, out);
        for (size_t i = 0; i < per; ++i) fwrite(slots[(size_t)f * per + i].data(), 1, (size_t)lens[(size_t)f * per + i], out);
    }
    fwrite(ry.data(), 1, ly, out), fwrite(rcb.data(), 1, lc, out), fwrite(rcr.data(), 1, lc, out);
    fwrite(words.data(), 4, words.size(), out);
    fclose(out);
    return 0;
}
