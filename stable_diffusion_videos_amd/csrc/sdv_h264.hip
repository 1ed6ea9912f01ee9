// H.264 CAVLC intra encoder (sdv_hip.h "H.264 CAVLC intra encoder"): uint8 RGB frames in HBM -> mp4 samples in one packed buffer.
//
//   sdv_h264_planes_u8     frames -> Y / Cb / Cr planes, integer BT.601, edge-replicated to whole macroblocks
//   sdv_h264_encode_rows   planes -> one complete slice (4-byte length | NAL header | payload with emulation prevention) per macroblock
//                          row and frame, each in its own slot of the scratch buffer, plus its length
//   sdv_h264_encode_gops   planes -> the same slots, but picture k of a call is an IDR picture only when k % gop == 0 and a P picture
//                          (zero-motion inter prediction from the reconstruction of picture k - 1) otherwise; reconstruction planes
//   sdv_h264_motion_search, sdv_h264_encode_gop_step (sdv_hip_ext.h "H.264 motion search")
//                          one even whole-sample vector per macroblock of every P picture from source luma; the GOP path one picture
//                          position per launch with those vectors
//   sdv_h264_motion_search_sub, sdv_h264_encode_gop_step_sub (sdv_hip_h264_sub.h "H.264 sub-sample motion")
//                          the same pair with vectors in quarter samples: odd whole, half and quarter samples, 6-tap luma and bilinear
//                          chroma prediction from clamped LDS windows
//   sdv_h264_encode_idr4 (sdv_hip_h264_i4.h "H.264 Intra4x4")
//                          the IDR pictures of a call with Intra4x4 prediction (I_NxN against Intra16x16 DC per macroblock), into the
//                          GOP path's slots; the P pictures then come from one of the two step entry points above
//   (sdv_h264_lf.hip, sdv_hip_h264_lf.h "H.264 deblocking": the in-loop deblocking filter and the _lf forms of the three per-position
//                          entry points; their kernels and this file's are the two forms of sdv_h264_step.h)
//   sdv_h264_pack          slots -> one contiguous buffer in sample order, and offsets[n + 1]
//   sdv_h264_vlc_tables    host only: the VLC tables of the kernel as (length, code) pairs
//
// Stream: one IDR slice per macroblock row, so the n * mbh rows are independent bit streams; inside a row every macroblock predicts from
// the reconstruction of the one before it - a serial chain.  One workgroup = one wave = one row: all lanes stage the macroblock's 384
// samples in LDS with 16- and 8-byte loads, lane 0 walks the chain (sdv_h264_core.h: transform, quantisation, CAVLC, the I_PCM decision,
// reconstruction of the right columns) with the levels in LDS.  The chains of a batch (4096 at 128 frames of 512 x 512) fill the GPU's
// wave slots; the work inside a chain is not spread over the lanes.
//
// GOP path: row r of picture k reads row r of the reconstruction of picture k - 1, so a chain is a (GOP, row) and there are gop times
// fewer of them.  One wave per chain again, but the macroblock's work is spread over its lanes: one 4x4 block per lane (16 luma, 8
// chroma) for SAD, residual, transform, quantisation and reconstruction, "any level nonzero" by ballot, levels and reconstruction in
// LDS; lane 0 keeps the DC blocks, the counting pass, the I_PCM decision and the bit writing.
#include "sdv_common.h"
#include "sdv_h264_core.h"
#include "sdv_hip_ext.h"
#include "sdv_hip_h264_sub.h"
#include "sdv_hip_h264_i4.h"
#include "sdv_h264_step.h"

namespace {

constexpr int kThreads = 256;

SDV_DEVICE int h264_luma(int r, int g, int b) { return ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16; }

// One thread per 2 x 2 samples of the padded planes.  Luma reads the pixel clamped into the frame; chroma reads the 2 x 2 box of the
// chroma position clamped into the frame's chroma grid - which is the edge replication of the finished planes.
__global__ __launch_bounds__(kThreads) void h264_planes_kernel(const uint8_t* __restrict__ frames, int H, int W, int ph, int pw,
                                                               uint8_t* __restrict__ y, uint8_t* __restrict__ cb, uint8_t* __restrict__ cr) {
    const int cw = pw / 2, chh = ph / 2;
    const int cx = blockIdx.x * kThreads + threadIdx.x, cy = blockIdx.y;
    const long long f = blockIdx.z;
    if (cx >= cw) return;
    const uint8_t* img = frames + f * H * W * 3;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int py = 2 * cy + (d >> 1), px = 2 * cx + (d & 1);
        const uint8_t* p = img + ((long long)min(py, H - 1) * W + min(px, W - 1)) * 3;
        y[(f * ph + py) * pw + px] = (uint8_t)h264_luma(p[0], p[1], p[2]);
    }
    const int sy = min(cy, H / 2 - 1), sx = min(cx, W / 2 - 1);
    int rs = 0, gs = 0, bs = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint8_t* p = img + ((long long)(2 * sy + (d >> 1)) * W + 2 * sx + (d & 1)) * 3;
        rs += p[0], gs += p[1], bs += p[2];
    }
    cb[(f * chh + cy) * cw + cx] = (uint8_t)(((-38 * rs - 74 * gs + 112 * bs + 512) >> 10) + 128);
    cr[(f * chh + cy) * cw + cx] = (uint8_t)(((112 * rs - 94 * gs - 18 * bs + 512) >> 10) + 128);
}

__global__ __launch_bounds__(64) void h264_rows_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ cb, const uint8_t* __restrict__ cr,
                                                       int mbh, int mbw, int qp, int first_index, uint8_t* __restrict__ slots, long long stride,
                                                       long long slot_bytes, int32_t* __restrict__ lens) {
    __shared__ __attribute__((aligned(16))) uint8_t sy[256];
    __shared__ __attribute__((aligned(16))) uint8_t sc[128];
    __shared__ int16_t lev[kH264MbLevels];
    const int lane = threadIdx.x;
    const long long row = blockIdx.x;
    const int r = (int)(row % mbh);
    const long long f = row / mbh;
    uint8_t* slot = slots + row * stride;
    h264_writer w;
    h264_chain ch;
    w.init(slot + 5, slot_bytes - 5);
    ch.have = 0;
    if (lane == 0) h264_slice_header(w, (unsigned)(r * mbw), (unsigned)((first_index + f) & 1), qp);
    const uint8_t* yrow = y + (f * mbh + r) * 16 * ((long long)mbw * 16);
    const long long crow = (f * mbh + r) * 8 * ((long long)mbw * 8);
    for (int m = 0; m < mbw; ++m) {
        if (lane < 16) {
            *(uint4*)(sy + lane * 16) = *(const uint4*)(yrow + (long long)lane * (mbw * 16) + m * 16);
        } else if (lane < 32) {
            const int c = (lane - 16) >> 3, i = (lane - 16) & 7;
            *(uint2*)(sc + c * 64 + i * 8) = *(const uint2*)((c ? cr : cb) + crow + (long long)i * (mbw * 8) + m * 8);
        }
        __syncthreads();
        if (lane == 0) h264_encode_mb(sy, sc, lev, ch, qp, w);
        __syncthreads();
    }
    if (lane == 0) {
        w.put(1u, 1);                                   // rbsp_slice_trailing_bits
        while (w.n) w.put(0u, 1);
        const long long used = min(w.pos, slot_bytes - 5);      // (the capacity bound keeps pos below it; nothing was stored beyond)
        const unsigned len = (unsigned)(1 + used);
        slot[0] = (uint8_t)(len >> 24), slot[1] = (uint8_t)(len >> 16), slot[2] = (uint8_t)(len >> 8), slot[3] = (uint8_t)len;
        slot[4] = 0x65;                                 // nal_ref_idc 3, nal_unit_type 5
        lens[row] = (int32_t)(5 + used);
    }
}

// One wave per (GOP, macroblock row): the GOP's pictures in order, in each the row's macroblocks.  ry / rcb / rcr are written by this
// wave for picture k and read back by it for picture k + 1 (the fence between two pictures orders the two).
__global__ __launch_bounds__(64) void h264_gops_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ cb, const uint8_t* __restrict__ cr,
                                                       int n, int mbh, int mbw, int qp, int gop, int first_index, uint8_t* ry, uint8_t* rcb,
                                                       uint8_t* rcr, uint8_t* __restrict__ slots, long long stride, long long slot_bytes,
                                                       int32_t* __restrict__ lens) {
    __shared__ h264_gop_mb mb;
    const int lane = threadIdx.x;
    const int r = (int)(blockIdx.x % mbh);
    const long long g = blockIdx.x / mbh;
    const long long lw = (long long)mbw * 16, cw = (long long)mbw * 8;
    h264_writer w;
    h264_chain ch;
    int skip_run = 0;
    w.init(slots, 0);
    ch.have = 0;
    for (int k = 0; k < gop; ++k) {
        const long long f = g * gop + k;
        if (f >= n) break;
        const bool p = k > 0;
        const long long row = f * mbh + r;
        uint8_t* slot = slots + row * stride;
        if (lane == 0) {
            w.init(slot + 5, slot_bytes - 5);
            ch.have = 0;
            skip_run = 0;
            if (p) h264_p_slice_header(w, (unsigned)(r * mbw), (unsigned)k, qp);
            else h264_slice_header(w, (unsigned)(r * mbw), (unsigned)((first_index + f) & 1), qp);
        }
        const long long yat = row * 16 * lw, cat = row * 8 * cw;                   // this row in picture f; picture f - 1 lies mbh rows before
        const long long yref = yat - (long long)mbh * 16 * lw, cref = cat - (long long)mbh * 8 * cw;
        for (int m = 0; m < mbw; ++m) {
            if (lane < 16) {
                *(uint4*)(mb.sy + lane * 16) = *(const uint4*)(y + yat + lane * lw + m * 16);
                if (p) *(uint4*)(mb.fy + lane * 16) = *(const uint4*)(ry + yref + lane * lw + m * 16);
            } else if (lane < 32) {
                const int c = (lane - 16) >> 3, i = (lane - 16) & 7;
                *(uint2*)(mb.sc + c * 64 + i * 8) = *(const uint2*)((c ? cr : cb) + cat + i * cw + m * 8);
                if (p) *(uint2*)(mb.fc + c * 64 + i * 8) = *(const uint2*)((c ? rcr : rcb) + cref + i * cw + m * 8);
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
                const bool any_cdc = h264_gop_dc(&mb, inter, qp);
                h264_gop_serial(&mb, nz, any_cdc, inter, p, ch, w, &skip_run);
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
            if (p && skip_run) h264_put_ue(w, (unsigned)skip_run);                 // the slice ends in skipped macroblocks
            w.put(1u, 1);                               // rbsp_slice_trailing_bits
            while (w.n) w.put(0u, 1);
            const long long used = min(w.pos, slot_bytes - 5);      // (the capacity bound keeps pos below it; nothing was stored beyond)
            const unsigned len = (unsigned)(1 + used);
            slot[0] = (uint8_t)(len >> 24), slot[1] = (uint8_t)(len >> 16), slot[2] = (uint8_t)(len >> 8), slot[3] = (uint8_t)len;
            slot[4] = p ? 0x41 : 0x65;                  // nal_ref_idc 2, nal_unit_type 1 | nal_ref_idc 3, nal_unit_type 5
            lens[row] = (int32_t)(5 + used);
        }
        __threadfence();                                // the reconstruction of picture f is the reference of picture f + 1
        __syncthreads();
    }
}

// Motion search (sdv_hip_ext.h "H.264 motion search"): one wave per macroblock of every picture of the call, source luma of picture f
// against source luma of picture f - 1.  The three macroblock columns around the block, 16 + 2 search rows of them, are staged in LDS with
// 16-byte loads (zeros outside the picture: no admitted candidate reads them); the current block sits in registers.  Lanes own candidates
// (lane, lane + 64, ...: at most 289), each a plain sum of byte SADs over aligned LDS words shifted into place, so no SAD crosses lanes;
// the winner is one wave-wide minimum of h264_me_key.  IDR pictures get zeros.
constexpr int kWinStride = 64;                          // 48 bytes of window, padded: 16-byte stores, and the fifth word of a row's read

__global__ __launch_bounds__(64) void h264_motion_search_kernel(const uint8_t* __restrict__ y, int mbh, int mbw, int qp, int gop, int search,
                                                                int16_t* __restrict__ mv, int32_t* __restrict__ sad) {
    __shared__ __attribute__((aligned(16))) uint8_t win[(16 + 2 * kH264SearchMax) * kWinStride];
    __shared__ __attribute__((aligned(16))) uint8_t cur[256];
    const int lane = threadIdx.x;
    const long long id = blockIdx.x;                    // (f * mbh + my) * mbw + mx
    const int mx = (int)(id % mbw), my = (int)(id / mbw % mbh);
    const long long f = id / mbw / mbh;
    if (f % gop == 0) {
        if (lane == 0) {
            mv[2 * id] = 0, mv[2 * id + 1] = 0;
            if (sad) sad[id] = 0;
        }
        return;
    }
    const long long lw = (long long)mbw * 16;
    const uint8_t* ref = y + (f - 1) * mbh * 16 * lw;
    const int rows = 16 + 2 * search, y0 = 16 * my - search;
    for (int i = lane; i < rows * 3; i += 64) {
        const int wr = i / 3, j = i % 3, py = y0 + wr, bx = mx - 1 + j;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (py >= 0 && py < 16 * mbh && bx >= 0 && bx < mbw) v = *(const uint4*)(ref + py * lw + bx * 16);
        *(uint4*)(win + wr * kWinStride + j * 16) = v;
    }
    if (lane < 16) *(uint4*)(cur + lane * 16) = *(const uint4*)(y + ((f * mbh + my) * 16 + lane) * lw + mx * 16);
    __syncthreads();
    uint32_t c[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) c[i] = ((const uint32_t*)cur)[i];
    const int per = search + 1, lambda = h264_me_lambda(qp);
    unsigned best = 0xffffffffu;
    for (int ci = lane; ci < per * per; ci += 64) {
        const int vy = 2 * (ci / per) - search, vx = 2 * (ci % per) - search;
        if (!h264_mv_valid(vx, vy, search, mx, my, mbw, mbh)) continue;
        const int col = 16 + vx, shift = col & 3;      // 0 or 2: the window's words are aligned, the candidate's samples may not be
        const uint32_t* q = (const uint32_t*)(win + (search + vy) * kWinStride + (col & ~3));
        unsigned s = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            uint32_t w[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) w[j] = q[i * (kWinStride / 4) + j];
#pragma unroll
            for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w[j + 1], w[j], (unsigned)shift), c[i * 4 + j], s);
        }
        best = min(best, h264_me_key(h264_me_cost((int)s, lambda, vx, vy), vx, vy));
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o));
    if (lane == 0) {                                    // (0, 0) is always admitted, so there is a winner
        int cost, vx, vy;
        h264_me_unkey(best, &cost, &vx, &vy);
        mv[2 * id] = (int16_t)vx, mv[2 * id + 1] = (int16_t)vy;
        if (sad) sad[id] = cost - h264_me_cost(0, lambda, vx, vy);
    }
}

// ONE workgroup: exclusive scan of the slice lengths, frame-major -> starts[row], offsets[frame], offsets[n]
__global__ __launch_bounds__(kThreads) void h264_scan_kernel(const int32_t* __restrict__ lens, long long* __restrict__ starts, long long rows, int mbh,
                                                             long long* __restrict__ offsets) {
    __shared__ long long wsum[kThreads / 64];
    __shared__ long long running;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) running = 0;
    __syncthreads();
    for (long long i0 = 0; i0 < rows; i0 += kThreads) {
        const long long i = i0 + tid;
        const long long mine = i < rows ? (long long)lens[i] : 0;
        long long incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        long long before = running;
        for (int k = 0; k < wave; ++k) before += wsum[k];
        if (i < rows) {
            starts[i] = before + incl - mine;
            if (i % mbh == 0) offsets[i / mbh] = before + incl - mine;
        }
        __syncthreads();
        if (tid == kThreads - 1) running = before + incl;
        __syncthreads();
    }
    if (tid == 0) offsets[rows / mbh] = running;
}

__global__ __launch_bounds__(kThreads) void h264_copy_kernel(const uint8_t* __restrict__ slots, long long stride, const int32_t* __restrict__ lens,
                                                             const long long* __restrict__ starts, uint8_t* __restrict__ out, long long out_cap) {
    const long long row = blockIdx.x;
    const uint8_t* src = slots + row * stride;
    const long long at = starts[row];
    const int len = lens[row];
    for (int i = threadIdx.x; i < len; i += kThreads)
        if (at + i < out_cap) out[at + i] = src[i];
}

// Sub-sample motion search (sdv_hip_h264_sub.h "H.264 sub-sample motion"): one wave per macroblock again, vectors in quarter samples.
// The window holds the samples 16 mx - 20 .. 16 mx + 35 of 16 + 2 search + 5 rows that start search + 2 above the block, read with
// CLAMPED coordinates (an aligned word lies wholly inside or wholly outside the picture: outside it repeats the row's edge sample), so
// that a fractional candidate at the picture edge finds its filter taps.  Stage 1 is h264_motion_search_kernel's form over every whole
// sample (shift 0 .. 3, at most 18 candidates a lane).  Stages 2 and 3 take their at most 8 new candidates one after the other: lanes own
// 4 of the 256 samples, interpolate each straight from the window (h264_sub_luma), and one wave-wide sum gives the SAD to every lane, so
// the winner is picked uniformly.  The order is h264_sub_key, a 64-bit word.
constexpr int kSubWinStride = 64;                       // 56 bytes of window, padded
constexpr int kSubWinLeft = 20;                         // the window's first column lies this far left of the block: >= search + 2, a multiple of 4
constexpr int kSubWinRows = 16 + 2 * kH264SearchMax + 5;

SDV_DEVICE unsigned long long h264_wave_min64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned long long other = __shfl_xor(v, o);
        v = other < v ? other : v;
    }
    return v;
}

__global__ __launch_bounds__(64) void h264_motion_search_sub_kernel(const uint8_t* __restrict__ y, int mbh, int mbw, int qp, int gop, int search,
                                                                    int subpel, int16_t* __restrict__ mv, int32_t* __restrict__ sad) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kSubWinRows * kSubWinStride];
    __shared__ __attribute__((aligned(16))) uint8_t cur[256];
    const int lane = threadIdx.x;
    const long long id = blockIdx.x;                    // (f * mbh + my) * mbw + mx
    const int mx = (int)(id % mbw), my = (int)(id / mbw % mbh);
    const long long f = id / mbw / mbh;
    if (f % gop == 0) {
        if (lane == 0) {
            mv[2 * id] = 0, mv[2 * id + 1] = 0;
            if (sad) sad[id] = 0;
        }
        return;
    }
    const long long lw = (long long)mbw * 16;
    const uint8_t* ref = y + (f - 1) * mbh * 16 * lw;
    const int rows = 16 + 2 * search + 5, y0 = 16 * my - search - 2, x0 = 16 * mx - kSubWinLeft;
    for (int i = lane; i < rows * 14; i += 64) {
        const int wr = i / 14, j = i % 14, px = x0 + 4 * j;
        const uint8_t* line = ref + (long long)h264_sub_clampi(y0 + wr, 16 * mbh - 1) * lw;
        const uint32_t v = px < 0 ? line[0] * 0x01010101u : px >= 16 * mbw ? line[16 * mbw - 1] * 0x01010101u : *(const uint32_t*)(line + px);
        *(uint32_t*)(win + wr * kSubWinStride + 4 * j) = v;
    }
    if (lane < 16) *(uint4*)(cur + lane * 16) = *(const uint4*)(y + ((f * mbh + my) * 16 + lane) * lw + mx * 16);
    __syncthreads();
    const int lambda = h264_me_lambda(qp);
    unsigned long long best = ~0ull;
    {
        uint32_t c[64];
#pragma unroll
        for (int i = 0; i < 64; ++i) c[i] = ((const uint32_t*)cur)[i];
        const int per = 2 * search + 1;
        for (int ci = lane; ci < per * per; ci += 64) {
            const int vy = ci / per - search, vx = ci % per - search;              // whole samples
            if (!h264_sub_valid(4 * vx, 4 * vy, search, 1, mx, my, mbw, mbh)) continue;
            const int col = kSubWinLeft + vx, shift = col & 3;
            const uint32_t* q = (const uint32_t*)(win + (search + 2 + vy) * kSubWinStride + (col & ~3));
            unsigned s = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                uint32_t w[5];
#pragma unroll
                for (int j = 0; j < 5; ++j) w[j] = q[i * (kSubWinStride / 4) + j];
#pragma unroll
                for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w[j + 1], w[j], (unsigned)shift), c[i * 4 + j], s);
            }
            const unsigned long long key = h264_sub_key(h264_sub_cost((int)s, lambda, 4 * vx, 4 * vy), 4 * vx, 4 * vy);
            best = key < best ? key : best;
        }
    }
    best = h264_wave_min64(best);                       // (0, 0) is always admitted, so there is a winner
    const int r = lane >> 2, c0 = 4 * (lane & 3);       // stages 2 and 3: this lane's four samples
    for (int step = 2; step * subpel >= 4; step >>= 1) {
        int cost, cx, cy;
        h264_sub_unkey(best, &cost, &cx, &cy);
        for (int d = 0; d < 9; ++d) {
            const int vx = cx + step * (d % 3 - 1), vy = cy + step * (d / 3 - 1);
            if (d == 4 || !h264_sub_valid(vx, vy, search, subpel, mx, my, mbw, mbh)) continue;
            const uint8_t* g = win + (search + 2 + (vy >> 2) + r) * kSubWinStride + kSubWinLeft + (vx >> 2) + c0;
            int s = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int diff = (int)cur[r * 16 + c0 + e] - h264_sub_luma(g + e, kSubWinStride, vx & 3, vy & 3);
                s += diff < 0 ? -diff : diff;
            }
            s = h264_wave_sum(s);
            const unsigned long long key = h264_sub_key(h264_sub_cost(s, lambda, vx, vy), vx, vy);
            best = key < best ? key : best;
        }
    }
    if (lane == 0) {
        int cost, vx, vy;
        h264_sub_unkey(best, &cost, &vx, &vy);
        mv[2 * id] = (int16_t)vx, mv[2 * id + 1] = (int16_t)vy;
        if (sad) sad[id] = cost - h264_sub_cost(0, lambda, vx, vy);
    }
}

}  // namespace

extern "C" int sdv_h264_planes_u8(const uint8_t* frames, int32_t n, int32_t H, int32_t W, uint8_t* y, uint8_t* cb, uint8_t* cr, void* stream) {
    SDV_REQUIRE(frames && y && cb && cr, "sdv_h264_planes_u8: null pointer");
    SDV_REQUIRE(n > 0 && n <= 65535, "sdv_h264_planes_u8: bad frame count n=%d (1 .. 65535)", n);
    SDV_REQUIRE(H >= 2 && H <= 16384 && W >= 2 && W <= 16384 && H % 2 == 0 && W % 2 == 0,
                "sdv_h264_planes_u8: bad frame size H=%d W=%d (even, 2 .. 16384)", H, W);
    const int ph = (H + 15) / 16 * 16, pw = (W + 15) / 16 * 16;
    hipLaunchKernelGGL(h264_planes_kernel, dim3((unsigned)((pw / 2 + kThreads - 1) / kThreads), (unsigned)(ph / 2), (unsigned)n), dim3(kThreads), 0,
                       (hipStream_t)stream, frames, H, W, ph, pw, y, cb, cr);
    SDV_CHECK_LAUNCH("sdv_h264_planes_u8");
    return SDV_OK;
}

extern "C" int sdv_h264_encode_rows(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                    int32_t first_index, void* scratch, int64_t scratch_bytes, void* stream) {
    SDV_REQUIRE(y && cb && cr && scratch, "sdv_h264_encode_rows: null pointer");
    H264_GRID_ARGS("sdv_h264_encode_rows");
    SDV_REQUIRE(qp >= 0 && qp <= 51, "sdv_h264_encode_rows: qp=%d outside 0 .. 51", qp);
    SDV_REQUIRE(first_index >= 0, "sdv_h264_encode_rows: negative first_index");
    const h264_layout l = h264_scratch_layout(n, mbh, mbw);
    SDV_REQUIRE(scratch_bytes >= l.bytes, "sdv_h264_encode_rows: scratch buffer too small: %lld bytes, %lld slices of %d macroblocks need %lld",
                (long long)scratch_bytes, l.rows, mbw, l.bytes);
    SDV_REQUIRE((((uintptr_t)y) & 15) == 0 && (((uintptr_t)cb) & 7) == 0 && (((uintptr_t)cr) & 7) == 0 && (((uintptr_t)scratch) & 7) == 0,
                "sdv_h264_encode_rows: y must be 16-byte, cb / cr / scratch 8-byte aligned");
    uint8_t* base = (uint8_t*)scratch;
    hipLaunchKernelGGL(h264_rows_kernel, dim3((unsigned)l.rows), dim3(64), 0, (hipStream_t)stream, y, cb, cr, mbh, mbw, qp, first_index, base, l.stride,
                       l.slot, (int32_t*)(base + l.lens_at));
    SDV_CHECK_LAUNCH("sdv_h264_encode_rows");
    return SDV_OK;
}

extern "C" int sdv_h264_encode_gops(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                    int32_t gop, int32_t first_index, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch,
                                    int64_t scratch_bytes, void* stream) {
    SDV_REQUIRE(y && cb && cr && ry && rcb && rcr && scratch, "sdv_h264_encode_gops: null pointer");
    H264_GRID_ARGS("sdv_h264_encode_gops");
    SDV_REQUIRE(mbw <= 1008, "sdv_h264_encode_gops: mbw=%d above 1008 (its slots are those of a wider picture, which must stay within 1024)", mbw);
    SDV_REQUIRE(qp >= 0 && qp <= 51, "sdv_h264_encode_gops: qp=%d outside 0 .. 51", qp);
    SDV_REQUIRE(gop >= 1 && gop <= kH264GopMax, "sdv_h264_encode_gops: gop=%d outside 1 .. %d", gop, (int)kH264GopMax);
    SDV_REQUIRE(first_index >= 0, "sdv_h264_encode_gops: negative first_index");
    const h264_layout l = h264_scratch_layout(n, mbh, h264_gop_slot_mbw(mbw));
    SDV_REQUIRE(scratch_bytes >= l.bytes, "sdv_h264_encode_gops: scratch buffer too small: %lld bytes, %lld slices of %d macroblocks need %lld",
                (long long)scratch_bytes, l.rows, mbw, l.bytes);
    SDV_REQUIRE((((uintptr_t)y) & 15) == 0 && (((uintptr_t)cb) & 7) == 0 && (((uintptr_t)cr) & 7) == 0 && (((uintptr_t)scratch) & 7) == 0,
                "sdv_h264_encode_gops: y must be 16-byte, cb / cr / scratch 8-byte aligned");
    SDV_REQUIRE((((uintptr_t)ry) & 15) == 0 && (((uintptr_t)rcb) & 7) == 0 && (((uintptr_t)rcr) & 7) == 0,
                "sdv_h264_encode_gops: ry must be 16-byte, rcb / rcr 8-byte aligned");
    uint8_t* base = (uint8_t*)scratch;
    const long long chains = (long long)((n + gop - 1) / gop) * mbh;
    hipLaunchKernelGGL(h264_gops_kernel, dim3((unsigned)chains), dim3(64), 0, (hipStream_t)stream, y, cb, cr, n, mbh, mbw, qp, gop, first_index, ry, rcb,
                       rcr, base, l.stride, l.slot, (int32_t*)(base + l.lens_at));
    SDV_CHECK_LAUNCH("sdv_h264_encode_gops");
    return SDV_OK;
}

// ---- additive codec extensions of ABI 12 (include/sdv_hip_ext.h) ----
extern "C" int sdv_h264_motion_search(const uint8_t* y, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop, int32_t search, int16_t* mv,
                                      int32_t* sad, void* stream) {
    SDV_REQUIRE(y && mv, "sdv_h264_motion_search: null pointer");
    H264_GRID_ARGS("sdv_h264_motion_search");
    SDV_REQUIRE((long long)n * mbh * mbw < 0x7fffffffLL, "sdv_h264_motion_search: too many macroblocks for one grid");
    SDV_REQUIRE(qp >= 0 && qp <= 51, "sdv_h264_motion_search: qp=%d outside 0 .. 51", qp);
    SDV_REQUIRE(gop >= 1 && gop <= kH264GopMax, "sdv_h264_motion_search: gop=%d outside 1 .. %d", gop, (int)kH264GopMax);
    SDV_REQUIRE(search >= 2 && search <= kH264SearchMax && search % 2 == 0, "sdv_h264_motion_search: search=%d must be even, 2 .. %d", search,
                (int)kH264SearchMax);
    SDV_REQUIRE((((uintptr_t)y) & 15) == 0 && (((uintptr_t)mv) & 3) == 0 && (((uintptr_t)sad) & 3) == 0,
                "sdv_h264_motion_search: y must be 16-byte, mv / sad 4-byte aligned");
    hipLaunchKernelGGL(h264_motion_search_kernel, dim3((unsigned)((long long)n * mbh * mbw)), dim3(64), 0, (hipStream_t)stream, y, mbh, mbw, qp, gop,
                       search, mv, sad);
    SDV_CHECK_LAUNCH("sdv_h264_motion_search");
    return SDV_OK;
}

extern "C" int sdv_h264_encode_gop_step(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                        int32_t gop, int32_t k, int32_t search, int32_t first_index, const int16_t* mv, uint8_t* ry, uint8_t* rcb,
                                        uint8_t* rcr, void* scratch, int64_t scratch_bytes, void* stream) {
    return h264_encode_gop_step_impl<false>(y, cb, cr, n, mbh, mbw, qp, gop, k, search, first_index, mv, ry, rcb, rcr, scratch, scratch_bytes, nullptr, stream);
}

// ---- sub-sample motion (include/sdv_hip_h264_sub.h): the two entry points above with vectors in quarter samples ----
extern "C" int sdv_h264_motion_search_sub(const uint8_t* y, int32_t n, int32_t mbh, int32_t mbw, int32_t qp, int32_t gop, int32_t search,
                                          int32_t subpel, int16_t* mv, int32_t* sad, void* stream) {
    SDV_REQUIRE(y && mv, "sdv_h264_motion_search_sub: null pointer");
    H264_GRID_ARGS("sdv_h264_motion_search_sub");
    SDV_REQUIRE((long long)n * mbh * mbw < 0x7fffffffLL, "sdv_h264_motion_search_sub: too many macroblocks for one grid");
    SDV_REQUIRE(qp >= 0 && qp <= 51, "sdv_h264_motion_search_sub: qp=%d outside 0 .. 51", qp);
    SDV_REQUIRE(gop >= 1 && gop <= kH264GopMax, "sdv_h264_motion_search_sub: gop=%d outside 1 .. %d", gop, (int)kH264GopMax);
    SDV_REQUIRE(search >= 2 && search <= kH264SearchMax && search % 2 == 0, "sdv_h264_motion_search_sub: search=%d must be even, 2 .. %d", search,
                (int)kH264SearchMax);
    SDV_REQUIRE(h264_subpel_ok(subpel), "sdv_h264_motion_search_sub: subpel=%d must be 1, 2 or 4", subpel);
    SDV_REQUIRE((((uintptr_t)y) & 15) == 0 && (((uintptr_t)mv) & 3) == 0 && (((uintptr_t)sad) & 3) == 0,
                "sdv_h264_motion_search_sub: y must be 16-byte, mv / sad 4-byte aligned");
    hipLaunchKernelGGL(h264_motion_search_sub_kernel, dim3((unsigned)((long long)n * mbh * mbw)), dim3(64), 0, (hipStream_t)stream, y, mbh, mbw, qp,
                       gop, search, subpel, mv, sad);
    SDV_CHECK_LAUNCH("sdv_h264_motion_search_sub");
    return SDV_OK;
}

extern "C" int sdv_h264_encode_gop_step_sub(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                            int32_t gop, int32_t k, int32_t search, int32_t subpel, int32_t first_index, const int16_t* mv,
                                            uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch, int64_t scratch_bytes, void* stream) {
    return h264_encode_gop_step_sub_impl<false>(y, cb, cr, n, mbh, mbw, qp, gop, k, search, subpel, first_index, mv, ry, rcb, rcr, scratch, scratch_bytes,
                                         nullptr, stream);
}

// ---- Intra4x4 IDR pictures (include/sdv_hip_h264_i4.h): the pictures at positions k % gop == 0 of a call, into the GOP path's slots ----
extern "C" int sdv_h264_encode_idr4(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int32_t n, int32_t mbh, int32_t mbw, int32_t qp,
                                    int32_t gop, int32_t first_index, uint8_t* ry, uint8_t* rcb, uint8_t* rcr, void* scratch,
                                    int64_t scratch_bytes, void* stream) {
    return h264_encode_idr4_impl<false>(y, cb, cr, n, mbh, mbw, qp, gop, first_index, ry, rcb, rcr, scratch, scratch_bytes, nullptr, stream);
}

extern "C" int sdv_h264_pack(void* scratch, int64_t scratch_bytes, int32_t n, int32_t mbh, int32_t mbw, uint8_t* out, int64_t out_cap,
                             int64_t* offsets, void* stream) {
    SDV_REQUIRE(scratch && out && offsets, "sdv_h264_pack: null pointer");
    H264_GRID_ARGS("sdv_h264_pack");
    const h264_layout l = h264_scratch_layout(n, mbh, mbw);
    SDV_REQUIRE(scratch_bytes >= l.bytes, "sdv_h264_pack: scratch buffer too small: %lld bytes, %lld slices of %d macroblocks need %lld",
                (long long)scratch_bytes, l.rows, mbw, l.bytes);
    SDV_REQUIRE(out_cap >= l.rows * l.slot, "sdv_h264_pack: output capacity %lld below the bound %lld (%lld slices of at most %lld bytes)",
                (long long)out_cap, l.rows * l.slot, l.rows, l.slot);
    SDV_REQUIRE((((uintptr_t)scratch) & 7) == 0 && (((uintptr_t)offsets) & 7) == 0, "sdv_h264_pack: scratch / offsets must be 8-byte aligned");
    uint8_t* base = (uint8_t*)scratch;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(h264_scan_kernel, dim3(1), dim3(kThreads), 0, s, (const int32_t*)(base + l.lens_at), (long long*)(base + l.starts_at), l.rows, mbh,
                       (long long*)offsets);
    SDV_CHECK_LAUNCH("sdv_h264_pack (scan)");
    hipLaunchKernelGGL(h264_copy_kernel, dim3((unsigned)l.rows), dim3(kThreads), 0, s, (const uint8_t*)base, l.stride, (const int32_t*)(base + l.lens_at),
                       (const long long*)(base + l.starts_at), out, (long long)out_cap);
    SDV_CHECK_LAUNCH("sdv_h264_pack (copy)");
    return SDV_OK;
}

extern "C" int sdv_h264_vlc_tables(uint8_t* lengths, uint16_t* codes, int32_t count) {
    SDV_REQUIRE(lengths && codes, "sdv_h264_vlc_tables: null pointer");
    SDV_REQUIRE(count == kH264VlcWords, "sdv_h264_vlc_tables: the tables hold %d words, got room for %d", (int)kH264VlcWords, count);
    for (int i = 0; i < kH264VlcWords; ++i) {
        lengths[i] = (uint8_t)(kH264VlcHost[i] >> 8);
        codes[i] = (uint16_t)(kH264VlcHost[i] & 0xffu);
    }
    return SDV_OK;
}
