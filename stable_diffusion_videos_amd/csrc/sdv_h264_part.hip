// Macroblock partitions of the H.264 track (sdv_hip_h264_part.h "H.264 partitions"): the search that keeps four quadrant winners beside the
// 16x16 one, the per-position encode kernel that reads four vectors a macroblock (with and without the loop filter's side information),
// and the filter with four vectors a side.  A unit of its own: sdv_h264.hip and sdv_h264_lf.hip compile what they compiled before (the
// kernel templates of sdv_h264_step.h are not instantiated here; only its helpers and launch checks are used).
#include "sdv_common.h"
#include "sdv_h264_core.h"
#include "sdv_hip_h264_part.h"
#include "sdv_h264_step.h"

namespace {

// The search window of h264_motion_search_sub_kernel (sdv_h264.hip): samples 16 mx - 20 .. 16 mx + 35 of 16 + 2 search + 5 rows that start
// search + 2 above the block, read with clamped coordinates.
constexpr int kPartWinStride = 64;
constexpr int kPartWinLeft = 20;
constexpr int kPartWinRows = 16 + 2 * kH264SearchMax + 5;

SDV_DEVICE unsigned long long h264_part_wave_min64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned long long other = __shfl_xor(v, o);
        v = other < v ? other : v;
    }
    return v;
}

// One wave per macroblock.  Stage 1: lanes own candidates (every whole-sample vector; with subpel 0 the even ones), and keep the minimum
// of five keys - the 16x16 block and its four 8x8 quadrants, whose SADs are the partial sums of the same 64 sad_u8 words.  Stages 2 and 3
// for the 16x16 winner are h264_motion_search_sub_kernel's (lanes own 4 of the 256 samples, one wave-wide sum a candidate).  For the
// quadrants the samples are dealt out again so that quadrant q is lanes 16 q .. 16 q + 15 (two lanes a row of 8 samples): the four
// refinements run side by side, each lane on its own quadrant's candidate, with 16-lane sums (xor 1, 2, 4, 8 stays inside the group).  A
// candidate that is not admitted is not skipped but replaced by the centre and its key discarded, so every shuffle is in uniform flow.
__global__ __launch_bounds__(64) void h264_motion_search_part_kernel(const uint8_t* __restrict__ y, int mbh, int mbw, int qp, int gop, int search,
                                                                     int subpel, int16_t* __restrict__ mv, int32_t* __restrict__ sad) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kPartWinRows * kPartWinStride];
    __shared__ __attribute__((aligned(16))) uint8_t cur[256];
    const int lane = threadIdx.x;
    const long long id = blockIdx.x;                    // (f * mbh + my) * mbw + mx
    const int mx = (int)(id % mbw), my = (int)(id / mbw % mbh);
    const long long f = id / mbw / mbh;
    if (f % gop == 0) {
        if (lane < 8) mv[8 * id + lane] = 0;
        if (sad && lane < 5) sad[5 * id + lane] = 0;
        return;
    }
    const long long lw = (long long)mbw * 16;
    const uint8_t* ref = y + (f - 1) * mbh * 16 * lw;
    const int rows = 16 + 2 * search + 5, y0 = 16 * my - search - 2, x0 = 16 * mx - kPartWinLeft;
    for (int i = lane; i < rows * 14; i += 64) {
        const int wr = i / 14, j = i % 14, px = x0 + 4 * j;
        const uint8_t* line = ref + (long long)h264_sub_clampi(y0 + wr, 16 * mbh - 1) * lw;
        const uint32_t v = px < 0 ? line[0] * 0x01010101u : px >= 16 * mbw ? line[16 * mbw - 1] * 0x01010101u : *(const uint32_t*)(line + px);
        *(uint32_t*)(win + wr * kPartWinStride + 4 * j) = v;
    }
    if (lane < 16) *(uint4*)(cur + lane * 16) = *(const uint4*)(y + ((f * mbh + my) * 16 + lane) * lw + mx * 16);
    __syncthreads();
    const int lambda = h264_me_lambda(qp);
    unsigned long long best16 = ~0ull, b0 = ~0ull, b1 = ~0ull, b2 = ~0ull, b3 = ~0ull;
    {
        uint32_t c[64];
#pragma unroll
        for (int i = 0; i < 64; ++i) c[i] = ((const uint32_t*)cur)[i];
        const int step1 = subpel ? 1 : 2, per = 2 * search / step1 + 1;
        for (int ci = lane; ci < per * per; ci += 64) {
            const int vy = step1 * (ci / per) - search, vx = step1 * (ci % per) - search;      // whole samples
            if (!h264_part_valid(4 * vx, 4 * vy, search, subpel ? 1 : 0, mx, my, mbw, mbh)) continue;
            const int col = kPartWinLeft + vx, shift = col & 3;
            const uint32_t* q = (const uint32_t*)(win + (search + 2 + vy) * kPartWinStride + (col & ~3));
            unsigned s[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                uint32_t w[5];
#pragma unroll
                for (int j = 0; j < 5; ++j) w[j] = q[i * (kPartWinStride / 4) + j];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    s[2 * (i >> 3) + (j >> 1)] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w[j + 1], w[j], (unsigned)shift), c[i * 4 + j],
                                                                         s[2 * (i >> 3) + (j >> 1)]);
            }
            const int bits = lambda * (h264_se_bits(4 * vx) + h264_se_bits(4 * vy));
            const unsigned long long k16 = h264_sub_key((int)(s[0] + s[1] + s[2] + s[3]) + bits, 4 * vx, 4 * vy);
            const unsigned long long k0 = h264_sub_key((int)s[0] + bits, 4 * vx, 4 * vy), k1 = h264_sub_key((int)s[1] + bits, 4 * vx, 4 * vy);
            const unsigned long long k2 = h264_sub_key((int)s[2] + bits, 4 * vx, 4 * vy), k3 = h264_sub_key((int)s[3] + bits, 4 * vx, 4 * vy);
            best16 = k16 < best16 ? k16 : best16;
            b0 = k0 < b0 ? k0 : b0, b1 = k1 < b1 ? k1 : b1, b2 = k2 < b2 ? k2 : b2, b3 = k3 < b3 ? k3 : b3;
        }
    }
    best16 = h264_part_wave_min64(best16);              // (0, 0) is always admitted, so there are winners
    b0 = h264_part_wave_min64(b0), b1 = h264_part_wave_min64(b1), b2 = h264_part_wave_min64(b2), b3 = h264_part_wave_min64(b3);
    {
        const int r = lane >> 2, c0 = 4 * (lane & 3);   // the 16x16 refinement: this lane's four samples
        for (int step = 2; step * subpel >= 4; step >>= 1) {
            int cost, cx, cy;
            h264_sub_unkey(best16, &cost, &cx, &cy);
            for (int d = 0; d < 9; ++d) {
                const int vx = cx + step * (d % 3 - 1), vy = cy + step * (d / 3 - 1);
                if (d == 4 || !h264_sub_valid(vx, vy, search, subpel, mx, my, mbw, mbh)) continue;
                const uint8_t* g = win + (search + 2 + (vy >> 2) + r) * kPartWinStride + kPartWinLeft + (vx >> 2) + c0;
                int s = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int diff = (int)cur[r * 16 + c0 + e] - h264_sub_luma(g + e, kPartWinStride, vx & 3, vy & 3);
                    s += diff < 0 ? -diff : diff;
                }
                s = h264_wave_sum(s);
                const unsigned long long key = h264_sub_key(h264_sub_cost(s, lambda, vx, vy), vx, vy);
                best16 = key < best16 ? key : best16;
            }
        }
    }
    const int quad = lane >> 4, t = lane & 15;
    unsigned long long mine = quad == 0 ? b0 : quad == 1 ? b1 : quad == 2 ? b2 : b3;
    {
        const int r = 8 * (quad >> 1) + (t >> 1), c0 = 8 * (quad & 1) + 4 * (t & 1);   // the quadrant refinements: this lane's four samples
        for (int step = 2; step * subpel >= 4; step >>= 1) {
            int cost, cx, cy;
            h264_sub_unkey(mine, &cost, &cx, &cy);
            for (int d = 0; d < 9; ++d) {
                const int vx = cx + step * (d % 3 - 1), vy = cy + step * (d / 3 - 1);
                const bool ok = d != 4 && h264_sub_valid(vx, vy, search, subpel, mx, my, mbw, mbh);
                const int ux = ok ? vx : cx, uy = ok ? vy : cy;                    // (the centre is admitted: its reads stay inside the window)
                const uint8_t* g = win + (search + 2 + (uy >> 2) + r) * kPartWinStride + kPartWinLeft + (ux >> 2) + c0;
                int s = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int diff = (int)cur[r * 16 + c0 + e] - h264_sub_luma(g + e, kPartWinStride, ux & 3, uy & 3);
                    s += diff < 0 ? -diff : diff;
                }
#pragma unroll
                for (int o = 8; o; o >>= 1) s += __shfl_xor(s, o);
                const unsigned long long key = ok ? h264_sub_key(h264_sub_cost(s, lambda, vx, vy), vx, vy) : ~0ull;
                mine = key < mine ? key : mine;
            }
        }
    }
    unsigned long long key8[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) key8[i] = __shfl(mine, 16 * i);
    if (lane == 0) {
        int out[4][2];
        h264_part_decide(key8, best16, lambda, out);
#pragma unroll
        for (int i = 0; i < 4; ++i) mv[8 * id + 2 * i] = (int16_t)out[i][0], mv[8 * id + 2 * i + 1] = (int16_t)out[i][1];
        if (sad) {
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                int cost, vx, vy;
                h264_sub_unkey(i < 4 ? key8[i] : best16, &cost, &vx, &vy);
                sad[5 * id + i] = cost - h264_sub_cost(0, lambda, vx, vy);
            }
        }
    }
}

// h264_gop_step_sub_kernel (sdv_h264_step.h) with four vectors a macroblock: for a P macroblock the four 13 x 13 luma windows and the
// 2 x 4 chroma windows of 5 x 5 of the reference RECONSTRUCTION are staged in LDS with clamped coordinates (no read leaves a plane,
// whatever the vectors), then every lane interpolates 4 luma and 2 chroma samples, each from the window of the partition it lies in.
// Whole-sample vectors take the same path: fraction 0 is a copy.  A vector of ``mv`` that is off the subpel grid, out of range or not
// admitted is coded as (0, 0) (h264_part_fetch), each partition for itself.  Everything after the prediction is that kernel's code with
// h264_gop_serial_part as the serial piece.  ``mbinfo`` null: the slice headers switch the loop filter off and nothing is stored; else
// they switch it on and lane 0 stores the macroblock's word (h264_part_lf_word).
__global__ __launch_bounds__(64) void h264_gop_step_part_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ cb, const uint8_t* __restrict__ cr,
                                                                int n, int mbh, int mbw, int qp, int gop, int k, int search, int subpel, int first_index,
                                                                const int16_t* __restrict__ mv, uint8_t* ry, uint8_t* rcb, uint8_t* rcr,
                                                                uint8_t* __restrict__ slots, long long stride, long long slot_bytes,
                                                                int32_t* __restrict__ lens, uint32_t* __restrict__ mbinfo) {
    constexpr int kLuma = kH264PartLumaWin * kH264PartLumaWin, kChroma = kH264PartChromaWin * kH264PartChromaWin;
    __shared__ h264_gop_mb mb;
    __shared__ uint8_t wy[4 * kLuma];
    __shared__ uint8_t wc[2 * 4 * kChroma];
    const int lane = threadIdx.x;
    const int r = (int)(blockIdx.x % mbh);
    const long long f = (long long)(blockIdx.x / mbh) * gop + k;
    if (f >= n) return;
    const long long lw = (long long)mbw * 16, cw = (long long)mbw * 8;
    const bool p = k > 0;
    const int lf = mbinfo ? 1 : 0;
    const long long row = f * mbh + r;
    uint8_t* slot = slots + row * stride;
    h264_writer w;
    h264_chain ch;
    h264_part_chain pc;
    int skip_run = 0;
    w.init(slot + 5, slot_bytes - 5);
    ch.have = 0;
    pc.v[0][0] = pc.v[0][1] = pc.v[1][0] = pc.v[1][1] = 0;
    if (lane == 0) {
        if (p) h264_p_slice_header(w, (unsigned)(r * mbw), (unsigned)k, qp, lf);
        else h264_slice_header(w, (unsigned)(r * mbw), (unsigned)((first_index + f) & 1), qp, lf);
    }
    const long long yat = row * 16 * lw, cat = row * 8 * cw;                       // this row in picture f
    const long long ypic = (f - 1) * mbh * 16 * lw, cpic = (f - 1) * mbh * 8 * cw;  // picture f - 1 (read in P pictures only)
    for (int m = 0; m < mbw; ++m) {
        h264_sub_ref at[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) at[i] = h264_part_fetch(0, 0, search, subpel, m, r, mbw, mbh);
        if (p) {
            const int16_t* v = mv + (row * mbw + m) * 8;
#pragma unroll
            for (int i = 0; i < 4; ++i) at[i] = h264_part_fetch(v[2 * i], v[2 * i + 1], search, subpel, m, r, mbw, mbh);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                for (int j = lane; j < kLuma; j += 64) wy[i * kLuma + j] = ry[ypic + h264_part_luma_at(at[i], i, j, m, r, mbw, mbh)];
                if (lane < 2 * kChroma) {
                    const int c = lane >= kChroma ? 1 : 0, j = lane - c * kChroma;
                    wc[(c * 4 + i) * kChroma + j] = (c ? rcr : rcb)[cpic + h264_part_chroma_at(at[i], i, j, m, r, mbw, mbh)];
                }
            }
            __syncthreads();
            {
                const int a = lane >> 2, b = 4 * (lane & 3);                       // luma: 4 samples of row a, all in one partition
                const int part = 2 * (a >> 3) + (b >> 3);
                const h264_sub_ref la = part == 0 ? at[0] : part == 1 ? at[1] : part == 2 ? at[2] : at[3];
                const uint8_t* g = wy + part * kLuma + ((a & 7) + 2) * kH264PartLumaWin + (b & 7) + 2;
#pragma unroll
                for (int e = 0; e < 4; ++e) mb.fy[a * 16 + b + e] = (uint8_t)h264_sub_luma(g + e, kH264PartLumaWin, la.xf, la.yf);
                const int c = lane >> 5, ca = (lane >> 2) & 7, cb2 = 2 * (lane & 3);   // chroma: 2 samples of row ca of component c
                const int cpart = 2 * (ca >> 2) + (cb2 >> 2);
                const h264_sub_ref lc = cpart == 0 ? at[0] : cpart == 1 ? at[1] : cpart == 2 ? at[2] : at[3];
                const uint8_t* ga = wc + (c * 4 + cpart) * kChroma + (ca & 3) * kH264PartChromaWin + (cb2 & 3);
#pragma unroll
                for (int e = 0; e < 2; ++e) mb.fc[c * 64 + ca * 8 + cb2 + e] = (uint8_t)h264_sub_chroma(ga + e, kH264PartChromaWin, lc.cxf, lc.cyf);
            }
        }
        if (lane < 16) {
            *(uint4*)(mb.sy + lane * 16) = *(const uint4*)(y + yat + lane * lw + m * 16);
        } else if (lane < 32) {
            const int c = (lane - 16) >> 3, i = (lane - 16) & 7;
            *(uint2*)(mb.sc + c * 64 + i * 8) = *(const uint2*)((c ? cr : cb) + cat + i * cw + m * 8);
        }
        if (lane == 0) h264_gop_pred(&mb, ch);
        __syncthreads();
        bool inter = false;
        if (p) {
            int si = 0, sp = 0;
            if (lane < 16) h264_gop_block_sad(&mb, lane, &si, &sp);
            si = h264_wave_sum(si), sp = h264_wave_sum(sp);
            inter = !(si < sp);
        }
        const bool mine = lane < 24 && h264_gop_block_forward(&mb, lane, inter, qp);
        const unsigned nz = (unsigned)__ballot(mine);
        __syncthreads();
        if (lane == 0) {
            int v[4][2];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i][0] = at[i].vx, v[i][1] = at[i].vy;
            const bool any_cdc = h264_gop_dc(&mb, inter, qp);
            h264_gop_serial_part(&mb, nz, any_cdc, inter, p, ch, pc, v, w, &skip_run);
            if (mbinfo) mbinfo[row * mbw + m] = h264_part_lf_word(mb.mode, nz, v);
        }
        __syncthreads();
        if (lane < 24) h264_gop_block_recon(&mb, lane, qp);
        __syncthreads();
        if (lane < 16) {
            *(uint4*)(ry + yat + lane * lw + m * 16) = *(const uint4*)(mb.ry + lane * 16);
        } else if (lane < 32) {
            const int c = (lane - 16) >> 3, i = (lane - 16) & 7;
            *(uint2*)((c ? rcr : rcb) + cat + i * cw + m * 8) = *(const uint2*)(mb.rc + c * 64 + i * 8);
        }
        if (lane == 0) h264_gop_chain(&mb, ch);
        __syncthreads();
    }
    if (lane == 0) {
        if (p && skip_run) h264_put_ue(w, (unsigned)skip_run);                     // the slice ends in skipped macroblocks
        w.put(1u, 1);                                   // rbsp_slice_trailing_bits
        while (w.n) w.put(0u, 1);
        const long long used = min(w.pos, slot_bytes - 5);      // (the capacity bound keeps pos below it; nothing was stored beyond)
        const unsigned len = (unsigned)(1 + used);
        slot[0] = (uint8_t)(len >> 24), slot[1] = (uint8_t)(len >> 16), slot[2] = (uint8_t)(len >> 8), slot[3] = (uint8_t)len;
        slot[4] = p ? 0x41 : 0x65;                      // nal_ref_idc 2, nal_unit_type 1 | nal_ref_idc 3, nal_unit_type 5
        lens[row] = (int32_t)(5 + used);
    }
}

// h264_deblock_kernel (sdv_h264_lf.hip) with four vectors a side: the same diagonals, windows, lanes and stores; only the sides and the
// line functions are the four-vector ones (h264_part_side_of, h264_part_luma_line, h264_part_chroma_line).
constexpr int kPartLfWaves = 16;
constexpr int kPartLfLumaStride = 32, kPartLfLumaAt = 4 * kPartLfLumaStride + 16;
constexpr int kPartLfChromaStride = 16, kPartLfChromaAt = 2 * kPartLfChromaStride + 8;
struct __attribute__((aligned(16))) h264_part_lf_window {
    uint8_t y[20 * kPartLfLumaStride];
    uint8_t c[2][10 * kPartLfChromaStride];
};

__global__ __launch_bounds__(kPartLfWaves * 64) void h264_deblock_part_kernel(uint8_t* ry, uint8_t* rcb, uint8_t* rcr, int n, int mbh, int mbw, int qp,
                                                                              int gop, int k, const uint32_t* __restrict__ mbinfo,
                                                                              const int16_t* __restrict__ mv) {
    __shared__ h264_part_lf_window win[kPartLfWaves];
    const long long f = (long long)blockIdx.x * gop + k;
    if (f >= n || qp < 16) return;                      // indexA <= qp < 16: alpha' = 0, no sample can change
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const long long lw = (long long)mbw * 16, cw = (long long)mbw * 8;
    uint8_t* py = ry + f * mbh * 16 * lw;
    uint8_t* pc[2] = {rcb + f * mbh * 8 * cw, rcr + f * mbh * 8 * cw};
    const uint32_t* info = mbinfo + f * mbh * mbw;
    const int16_t* vec = mv + f * mbh * mbw * 8;
    h264_part_lf_window& wn = win[wave];
    uint8_t* wy = wn.y + kPartLfLumaAt;
    for (int d = 0; d <= mbw - 1 + 2 * (mbh - 1); ++d) {
        const int ylo = d > mbw - 1 ? (d - mbw + 2) >> 1 : 0, yhi = min(mbh - 1, d >> 1);
        for (int i0 = 0; i0 <= yhi - ylo; i0 += waves) {
            const bool active = i0 + wave <= yhi - ylo;
            const int my = ylo + i0 + wave, mx = d - 2 * my;
            uint8_t* gy = py;
            uint8_t* gc[2] = {pc[0], pc[1]};
            h264_part_side q, left, up;
            q.info = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) q.v[i][0] = q.v[i][1] = 0;
            left = up = q;
            if (active) {
                const int at = my * mbw + mx;
                q = h264_part_side_of(info[at], vec + 8 * at);
                left = mx ? h264_part_side_of(info[at - 1], vec + 8 * (at - 1)) : q;
                up = my ? h264_part_side_of(info[at - mbw], vec + 8 * (at - mbw)) : q;
                gy += (long long)my * 16 * lw + mx * 16;
                gc[0] += (long long)my * 8 * cw + mx * 8, gc[1] += (long long)my * 8 * cw + mx * 8;
                if (lane < 16) {                        // the macroblock's luma rows
                    *(uint4*)(wy + lane * kPartLfLumaStride) = *(const uint4*)(gy + lane * lw);
                } else if (lane < 32) {                 // 4 columns of the left neighbour
                    const int l = lane - 16;
                    if (mx) *(uint32_t*)(wy + l * kPartLfLumaStride - 4) = *(const uint32_t*)(gy + l * lw - 4);
                } else if (lane < 36) {                 // 4 rows of the upper neighbour
                    const int l = lane - 36;            // -4 .. -1
                    if (my) *(uint4*)(wy + l * kPartLfLumaStride) = *(const uint4*)(gy + l * lw);
                } else if (lane < 52) {                 // the macroblock's chroma rows
                    const int c = (lane - 36) >> 3, l = (lane - 36) & 7;
                    *(uint2*)(wn.c[c] + kPartLfChromaAt + l * kPartLfChromaStride) = *(const uint2*)(gc[c] + l * cw);
                }
                if (lane < 16) {                        // 2 chroma columns of the left neighbour
                    const int c = lane >> 3, l = lane & 7;
                    if (mx) *(uint16_t*)(wn.c[c] + kPartLfChromaAt + l * kPartLfChromaStride - 2) = *(const uint16_t*)(gc[c] + l * cw - 2);
                } else if (lane < 20) {                 // 2 chroma rows of the upper neighbour
                    const int c = (lane - 16) >> 1, l = ((lane - 16) & 1) - 2;
                    if (my) *(uint2*)(wn.c[c] + kPartLfChromaAt + l * kPartLfChromaStride) = *(const uint2*)(gc[c] + l * cw);
                }
            }
            __syncthreads();
            for (int dir = 0; dir < 2; ++dir) {
                if (active) {
                    const bool edge0 = (dir ? my : mx) > 0;
                    const h264_part_side& nb = dir ? up : left;
                    if (lane < 16) {
                        for (int e = edge0 ? 0 : 1; e < 4; ++e) h264_part_luma_line(wy, kPartLfLumaStride, dir, e, lane, e ? q : nb, q, qp);
                    } else if (lane < 32) {
                        const int c = (lane - 16) >> 3, l = (lane - 16) & 7;
                        for (int e = edge0 ? 0 : 1; e < 2; ++e)
                            h264_part_chroma_line(wn.c[c] + kPartLfChromaAt, kPartLfChromaStride, dir, e, l, e ? q : nb, q, qp);
                    }
                }
                __syncthreads();
            }
            if (active) {
                if (lane < 16) {
                    *(uint4*)(gy + lane * lw) = *(const uint4*)(wy + lane * kPartLfLumaStride);
                } else if (lane < 32) {
                    const int l = lane - 16;
                    if (mx)
                        for (int j = -3; j < 0; ++j) gy[l * lw + j] = wy[l * kPartLfLumaStride + j];
                } else if (lane < 35) {
                    const int l = lane - 35;            // -3 .. -1
                    if (my) *(uint4*)(gy + l * lw) = *(const uint4*)(wy + l * kPartLfLumaStride);
                } else if (lane < 51) {
                    const int c = (lane - 35) >> 3, l = (lane - 35) & 7;
                    *(uint2*)(gc[c] + l * cw) = *(const uint2*)(wn.c[c] + kPartLfChromaAt + l * kPartLfChromaStride);
                }
                if (lane < 16) {
                    const int c = lane >> 3, l = lane & 7;
                    if (mx) gc[c][l * cw - 1] = wn.c[c][kPartLfChromaAt + l * kPartLfChromaStride - 1];
                } else if (lane < 18) {
                    const int c = lane - 16;
                    if (my) *(uint2*)(gc[c] - cw) = *(const uint2*)(wn.c[c] + kPartLfChromaAt - kPartLfChromaStride);
                }
            }
        }
        __threadfence_block();                          // this diagonal's stores before the next diagonal's loads, inside the workgroup
        __syncthreads();
    }
}

}  // namespace

#define H264_PART_MV_ARGS(name)                                                                                                          \
    SDV_REQUIRE(mv, name ": null pointer");                                                                                              \
    SDV_REQUIRE((((uintptr_t)mv) & 3) == 0, name ": mv must be 4-byte aligned");                                                         \
    SDV_REQUIRE(n > 0 && mbh > 0 && mbw > 0 && mv_count == (int64_t)n * mbh * mbw * 8,                                                    \
                name ": mv holds %lld elements, %d pictures of %d x %d macroblocks with four vectors have %lld", (long long)mv_count, n, mbh, \
                mbw, (long long)n * mbh * mbw * 8)
#define H264_PART_MBINFO_ARGS(name)                                                                                                      \
    SDV_REQUIRE(mbinfo, name ": null pointer");                                                                                          \
    SDV_REQUIRE((((uintptr_t)mbinfo) & 3) == 0, name ": mbinfo must be 4-byte aligned");                                                \
    SDV_REQUIRE(n > 0 && mbh > 0 && mbw > 0 && mbinfo_count == (int64_t)n * mbh * mbw,                                                   \
                name ": mbinfo holds %lld words, %d pictures of %d x %d macroblocks have %lld", (long long)mbinfo_count, n, mbh, mbw,    \
                (long long)n * mbh * mbw)

extern "C" int sdv_h264_motion_search_part(const uint8_t* y, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop, int32_t search,
                                           int32_t subpel, int16_t* mv, int64_t mv_count, int32_t* sad, int64_t sad_count, void* stream) {
    SDV_REQUIRE(y, "sdv_h264_motion_search_part: null pointer");
    H264_PART_MV_ARGS("sdv_h264_motion_search_part");
    H264_GRID_ARGS("sdv_h264_motion_search_part");
    SDV_REQUIRE((long long)n * mbh * mbw < 0x7fffffffLL, "sdv_h264_motion_search_part: too many macroblocks for one grid");
    SDV_REQUIRE(!sad || sad_count == (int64_t)n * mbh * mbw * 5, "sdv_h264_motion_search_part: sad holds %lld elements, five a macroblock are %lld",
                (long long)sad_count, (long long)n * mbh * mbw * 5);
    SDV_REQUIRE(qp >= 0 && qp <= 51, "sdv_h264_motion_search_part: qp=%d outside 0 .. 51", qp);
    SDV_REQUIRE(gop >= 1 && gop <= kH264GopMax, "sdv_h264_motion_search_part: gop=%d outside 1 .. %d", gop, (int)kH264GopMax);
    SDV_REQUIRE(search >= 2 && search <= kH264SearchMax && search % 2 == 0, "sdv_h264_motion_search_part: search=%d must be even, 2 .. %d", search,
                (int)kH264SearchMax);
    SDV_REQUIRE(h264_part_subpel_ok(subpel), "sdv_h264_motion_search_part: subpel=%d must be 0, 1, 2 or 4", subpel);
    SDV_REQUIRE((((uintptr_t)y) & 15) == 0 && (((uintptr_t)sad) & 3) == 0, "sdv_h264_motion_search_part: y must be 16-byte, sad 4-byte aligned");
    hipLaunchKernelGGL(h264_motion_search_part_kernel, dim3((unsigned)((long long)n * mbh * mbw)), dim3(64), 0, (hipStream_t)stream, y, mbh, mbw, qp,
                       gop, search, subpel, mv, sad);
    SDV_CHECK_LAUNCH("sdv_h264_motion_search_part");
    return SDV_OK;
}

static int h264_encode_gop_step_part_impl(const char* name, const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw,
                                          int32_t qp, int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv,
                                          int64_t mv_count, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes,
                                          uint32_t* mbinfo, void* stream) {
    SDV_REQUIRE(y && cb && cr && ry && rcb && rcr && scratch, "%s: null pointer", name);
    H264_PART_MV_ARGS("sdv_h264_encode_gop_step_part");
    H264_GRID_ARGS("sdv_h264_encode_gop_step_part");
    SDV_REQUIRE(mbw <= 1008, "%s: mbw=%d above 1008 (its slots are those of a wider picture, which must stay within 1024)", name, mbw);
    SDV_REQUIRE(qp >= 0 && qp <= 51, "%s: qp=%d outside 0 .. 51", name, qp);
    SDV_REQUIRE(gop >= 1 && gop <= kH264GopMax, "%s: gop=%d outside 1 .. %d", name, gop, (int)kH264GopMax);
    SDV_REQUIRE(k >= 0 && k < gop && k < n, "%s: position k=%d outside 0 .. min(gop, n) - 1 (gop=%d, n=%d)", name, k, gop, n);
    SDV_REQUIRE(search >= 2 && search <= kH264SearchMax && search % 2 == 0, "%s: search=%d must be even, 2 .. %d", name, search, (int)kH264SearchMax);
    SDV_REQUIRE(h264_part_subpel_ok(subpel), "%s: subpel=%d must be 0, 1, 2 or 4", name, subpel);
    SDV_REQUIRE(first_index >= 0, "%s: negative first_index", name);
    const h264_layout l = h264_scratch_layout(n, mbh, h264_gop_slot_mbw(mbw));
    SDV_REQUIRE(scratch_bytes >= l.bytes, "%s: scratch buffer too small: %lld bytes, %lld slices of %d macroblocks need %lld", name,
                (long long)scratch_bytes, l.rows, mbw, l.bytes);
    SDV_REQUIRE((((uintptr_t)y) & 15) == 0 && (((uintptr_t)cb) & 7) == 0 && (((uintptr_t)cr) & 7) == 0 && (((uintptr_t)scratch) & 7) == 0,
                "%s: y must be 16-byte, cb / cr / scratch 8-byte aligned", name);
    SDV_REQUIRE((((uintptr_t)ry) & 15) == 0 && (((uintptr_t)rcb) & 7) == 0 && (((uintptr_t)rcr) & 7) == 0, "%s: ry must be 16-byte, rcb / rcr 8-byte aligned",
                name);
    uint8_t* base = (uint8_t*)scratch;
    const long long chains = (long long)((n - k + gop - 1) / gop) * mbh;           // the GOPs that have a picture at position k
    hipLaunchKernelGGL(h264_gop_step_part_kernel, dim3((unsigned)chains), dim3(64), 0, (hipStream_t)stream, y, cb, cr, n, mbh, mbw, qp, gop, k, search,
                       subpel, first_index, mv, ry, rcb, rcr, base, l.stride, l.slot, (int32_t*)(base + l.lens_at), mbinfo);
    SDV_CHECK_LAUNCH(name);
    return SDV_OK;
}

extern "C" int sdv_h264_encode_gop_step_part(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                             int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv,
                                             int64_t mv_count, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes,
                                             void* stream) {
    return h264_encode_gop_step_part_impl("sdv_h264_encode_gop_step_part", y, cb, cr, n, mbh, mbw, qp, gop, k, search, subpel, first_index, mv, mv_count,
                                          ry, rcb, rcr, scratch, scratch_bytes, nullptr, stream);
}

extern "C" int sdv_h264_encode_gop_step_part_lf(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                                int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv,
                                                int64_t mv_count, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes,
                                                uint32_t* mbinfo, int64_t mbinfo_count, void* stream) {
    H264_PART_MBINFO_ARGS("sdv_h264_encode_gop_step_part_lf");
    return h264_encode_gop_step_part_impl("sdv_h264_encode_gop_step_part_lf", y, cb, cr, n, mbh, mbw, qp, gop, k, search, subpel, first_index, mv,
                                          mv_count, ry, rcb, rcr, scratch, scratch_bytes, mbinfo, stream);
}

extern "C" int sdv_h264_deblock_part(uint8_t* ry, uint8_t* rcb, uint8_t* rcr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop, int32_t k,
                                     const uint32_t* mbinfo, int64_t mbinfo_count, const int16_t* mv, int64_t mv_count, int32_t waves, void* stream) {
    SDV_REQUIRE(ry && rcb && rcr, "sdv_h264_deblock_part: null pointer");
    H264_PART_MBINFO_ARGS("sdv_h264_deblock_part");
    H264_PART_MV_ARGS("sdv_h264_deblock_part");
    H264_GRID_ARGS("sdv_h264_deblock_part");
    SDV_REQUIRE(qp >= 0 && qp <= 51, "sdv_h264_deblock_part: qp=%d outside 0 .. 51", qp);
    SDV_REQUIRE(gop >= 1 && gop <= kH264GopMax, "sdv_h264_deblock_part: gop=%d outside 1 .. %d", gop, (int)kH264GopMax);
    SDV_REQUIRE(k >= 0 && k < gop && k < n, "sdv_h264_deblock_part: position k=%d outside 0 .. min(gop, n) - 1 (gop=%d, n=%d)", k, gop, n);
    SDV_REQUIRE(waves >= 0 && waves <= kPartLfWaves, "sdv_h264_deblock_part: waves=%d outside 0 .. %d (0 = the default)", waves, (int)kPartLfWaves);
    SDV_REQUIRE((((uintptr_t)ry) & 15) == 0 && (((uintptr_t)rcb) & 7) == 0 && (((uintptr_t)rcr) & 7) == 0,
                "sdv_h264_deblock_part: ry must be 16-byte, rcb / rcr 8-byte aligned");
    const int longest = min(mbh, (mbw + 1) / 2);        // macroblocks on the longest diagonal x + 2 y
    const int use = waves ? waves : min((int)kPartLfWaves, longest);
    const long long pictures = (n - k + gop - 1) / gop; // the GOPs that have a picture at position k
    hipLaunchKernelGGL(h264_deblock_part_kernel, dim3((unsigned)pictures), dim3(64 * use), 0, (hipStream_t)stream, ry, rcb, rcr, n, mbh, mbw, qp, gop, k,
                       mbinfo, mv);
    SDV_CHECK_LAUNCH("sdv_h264_deblock_part");
    return SDV_OK;
}
