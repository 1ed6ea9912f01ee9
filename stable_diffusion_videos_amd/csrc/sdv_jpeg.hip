// Baseline JPEG encoder (sdv_hip.h "JPEG encoder"): uint8 RGB frames in HBM -> complete JFIF files in one packed buffer.
//
//   sdv_jpeg_transform_u8    frames -> quantised DCT coefficients, int16 [n][mcu_rows][mcu_cols][6][64] in zigzag order
//   sdv_jpeg_entropy_pack    coefficients -> header | Huffman-coded restart intervals | RSTm ... | EOI per frame, and offsets[n + 1]
//
// Stream: baseline sequential, 8 bit, 4:2:0 (MCU = 16 x 16 pixels = Y00 Y01 Y10 Y11 Cb Cr), the Annex K Huffman tables, ONE RESTART
// INTERVAL PER MCU ROW.  Every interval starts byte-aligned with its DC predictors at 0, so the n * mcu_rows intervals are independent
// Huffman streams: one wave each.
#include "sdv_common.h"

namespace {

// kDct[u * 8 + x] = c(u) / 2 * cos((2x + 1) u pi / 16), c(0) = 1 / sqrt 2: the orthonormal 8-point DCT-II
__constant__ const float kDct[64] = {
    0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f,
    0.490392625f, 0.415734798f, 0.277785122f, 0.0975451618f, -0.0975451618f, -0.277785122f, -0.415734798f, -0.490392625f,
    0.461939752f, 0.191341713f, -0.191341713f, -0.461939752f, -0.461939752f, -0.191341713f, 0.191341713f, 0.461939752f,
    0.415734798f, -0.0975451618f, -0.490392625f, -0.277785122f, 0.277785122f, 0.490392625f, 0.0975451618f, -0.415734798f,
    0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f, 0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f,
    0.277785122f, -0.490392625f, 0.0975451618f, 0.415734798f, -0.415734798f, -0.0975451618f, 0.490392625f, -0.277785122f,
    0.191341713f, -0.461939752f, 0.461939752f, -0.191341713f, -0.191341713f, 0.461939752f, -0.461939752f, 0.191341713f,
    0.0975451618f, -0.277785122f, 0.415734798f, -0.490392625f, 0.490392625f, -0.415734798f, 0.277785122f, -0.0975451618f,
};
// kZigzagPos[row * 8 + column] = position of that coefficient in the zigzag sequence (T.81 figure A.6)
__constant__ const uint8_t kZigzagPos[64] = {
    0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42,
    3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
    21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63,
};
// Annex K.3 - K.6 typical Huffman tables as (length << 16 | code), indexed by symbol: DC by size category, AC by run << 4 | size;
// 0 = no such symbol
__constant__ const uint32_t kHuff[544] = {
    0x020000u, 0x030002u, 0x030003u, 0x030004u, 0x030005u, 0x030006u, 0x04000eu, 0x05001eu,
    0x06003eu, 0x07007eu, 0x0800feu, 0x0901feu, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x020000u, 0x020001u, 0x020002u, 0x030006u, 0x04000eu, 0x05001eu, 0x06003eu, 0x07007eu,
    0x0800feu, 0x0901feu, 0x0a03feu, 0x0b07feu, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x04000au, 0x020000u, 0x020001u, 0x030004u, 0x04000bu, 0x05001au, 0x070078u, 0x0800f8u,
    0x0a03f6u, 0x10ff82u, 0x10ff83u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x04000cu, 0x05001bu, 0x070079u, 0x0901f6u, 0x0b07f6u, 0x10ff84u, 0x10ff85u,
    0x10ff86u, 0x10ff87u, 0x10ff88u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x05001cu, 0x0800f9u, 0x0a03f7u, 0x0c0ff4u, 0x10ff89u, 0x10ff8au, 0x10ff8bu,
    0x10ff8cu, 0x10ff8du, 0x10ff8eu, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x06003au, 0x0901f7u, 0x0c0ff5u, 0x10ff8fu, 0x10ff90u, 0x10ff91u, 0x10ff92u,
    0x10ff93u, 0x10ff94u, 0x10ff95u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x06003bu, 0x0a03f8u, 0x10ff96u, 0x10ff97u, 0x10ff98u, 0x10ff99u, 0x10ff9au,
    0x10ff9bu, 0x10ff9cu, 0x10ff9du, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x07007au, 0x0b07f7u, 0x10ff9eu, 0x10ff9fu, 0x10ffa0u, 0x10ffa1u, 0x10ffa2u,
    0x10ffa3u, 0x10ffa4u, 0x10ffa5u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x07007bu, 0x0c0ff6u, 0x10ffa6u, 0x10ffa7u, 0x10ffa8u, 0x10ffa9u, 0x10ffaau,
    0x10ffabu, 0x10ffacu, 0x10ffadu, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x0800fau, 0x0c0ff7u, 0x10ffaeu, 0x10ffafu, 0x10ffb0u, 0x10ffb1u, 0x10ffb2u,
    0x10ffb3u, 0x10ffb4u, 0x10ffb5u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x0901f8u, 0x0f7fc0u, 0x10ffb6u, 0x10ffb7u, 0x10ffb8u, 0x10ffb9u, 0x10ffbau,
    0x10ffbbu, 0x10ffbcu, 0x10ffbdu, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x0901f9u, 0x10ffbeu, 0x10ffbfu, 0x10ffc0u, 0x10ffc1u, 0x10ffc2u, 0x10ffc3u,
    0x10ffc4u, 0x10ffc5u, 0x10ffc6u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x0901fau, 0x10ffc7u, 0x10ffc8u, 0x10ffc9u, 0x10ffcau, 0x10ffcbu, 0x10ffccu,
    0x10ffcdu, 0x10ffceu, 0x10ffcfu, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x0a03f9u, 0x10ffd0u, 0x10ffd1u, 0x10ffd2u, 0x10ffd3u, 0x10ffd4u, 0x10ffd5u,
    0x10ffd6u, 0x10ffd7u, 0x10ffd8u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x0a03fau, 0x10ffd9u, 0x10ffdau, 0x10ffdbu, 0x10ffdcu, 0x10ffddu, 0x10ffdeu,
    0x10ffdfu, 0x10ffe0u, 0x10ffe1u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x0b07f8u, 0x10ffe2u, 0x10ffe3u, 0x10ffe4u, 0x10ffe5u, 0x10ffe6u, 0x10ffe7u,
    0x10ffe8u, 0x10ffe9u, 0x10ffeau, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x10ffebu, 0x10ffecu, 0x10ffedu, 0x10ffeeu, 0x10ffefu, 0x10fff0u, 0x10fff1u,
    0x10fff2u, 0x10fff3u, 0x10fff4u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x0b07f9u, 0x10fff5u, 0x10fff6u, 0x10fff7u, 0x10fff8u, 0x10fff9u, 0x10fffau, 0x10fffbu,
    0x10fffcu, 0x10fffdu, 0x10fffeu, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x020000u, 0x020001u, 0x030004u, 0x04000au, 0x050018u, 0x050019u, 0x060038u, 0x070078u,
    0x0901f4u, 0x0a03f6u, 0x0c0ff4u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x04000bu, 0x060039u, 0x0800f6u, 0x0901f5u, 0x0b07f6u, 0x0c0ff5u, 0x10ff88u,
    0x10ff89u, 0x10ff8au, 0x10ff8bu, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x05001au, 0x0800f7u, 0x0a03f7u, 0x0c0ff6u, 0x0f7fc2u, 0x10ff8cu, 0x10ff8du,
    0x10ff8eu, 0x10ff8fu, 0x10ff90u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x05001bu, 0x0800f8u, 0x0a03f8u, 0x0c0ff7u, 0x10ff91u, 0x10ff92u, 0x10ff93u,
    0x10ff94u, 0x10ff95u, 0x10ff96u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x06003au, 0x0901f6u, 0x10ff97u, 0x10ff98u, 0x10ff99u, 0x10ff9au, 0x10ff9bu,
    0x10ff9cu, 0x10ff9du, 0x10ff9eu, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x06003bu, 0x0a03f9u, 0x10ff9fu, 0x10ffa0u, 0x10ffa1u, 0x10ffa2u, 0x10ffa3u,
    0x10ffa4u, 0x10ffa5u, 0x10ffa6u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x070079u, 0x0b07f7u, 0x10ffa7u, 0x10ffa8u, 0x10ffa9u, 0x10ffaau, 0x10ffabu,
    0x10ffacu, 0x10ffadu, 0x10ffaeu, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x07007au, 0x0b07f8u, 0x10ffafu, 0x10ffb0u, 0x10ffb1u, 0x10ffb2u, 0x10ffb3u,
    0x10ffb4u, 0x10ffb5u, 0x10ffb6u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x0800f9u, 0x10ffb7u, 0x10ffb8u, 0x10ffb9u, 0x10ffbau, 0x10ffbbu, 0x10ffbcu,
    0x10ffbdu, 0x10ffbeu, 0x10ffbfu, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x0901f7u, 0x10ffc0u, 0x10ffc1u, 0x10ffc2u, 0x10ffc3u, 0x10ffc4u, 0x10ffc5u,
    0x10ffc6u, 0x10ffc7u, 0x10ffc8u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x0901f8u, 0x10ffc9u, 0x10ffcau, 0x10ffcbu, 0x10ffccu, 0x10ffcdu, 0x10ffceu,
    0x10ffcfu, 0x10ffd0u, 0x10ffd1u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x0901f9u, 0x10ffd2u, 0x10ffd3u, 0x10ffd4u, 0x10ffd5u, 0x10ffd6u, 0x10ffd7u,
    0x10ffd8u, 0x10ffd9u, 0x10ffdau, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x0901fau, 0x10ffdbu, 0x10ffdcu, 0x10ffddu, 0x10ffdeu, 0x10ffdfu, 0x10ffe0u,
    0x10ffe1u, 0x10ffe2u, 0x10ffe3u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x0b07f9u, 0x10ffe4u, 0x10ffe5u, 0x10ffe6u, 0x10ffe7u, 0x10ffe8u, 0x10ffe9u,
    0x10ffeau, 0x10ffebu, 0x10ffecu, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x000000u, 0x0e3fe0u, 0x10ffedu, 0x10ffeeu, 0x10ffefu, 0x10fff0u, 0x10fff1u, 0x10fff2u,
    0x10fff3u, 0x10fff4u, 0x10fff5u, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
    0x0a03fau, 0x0f7fc3u, 0x10fff6u, 0x10fff7u, 0x10fff8u, 0x10fff9u, 0x10fffau, 0x10fffbu,
    0x10fffcu, 0x10fffdu, 0x10fffeu, 0x000000u, 0x000000u, 0x000000u, 0x000000u, 0x000000u,
};
constexpr int kDcLuma = 0, kDcChroma = 16, kAcLuma = 32, kAcChroma = 32 + 256, kHuffWords = 32 + 512;

// ---------------------------------------------------------------------------------------------------------------------------
// Transform.  One workgroup = a strip of 16 rows x up to 16 MCUs (256 pixels) of one frame:
//   1. the strip's bytes -> LDS (16-byte loads when every row starts 16-byte aligned, i.e. W % 16 == 0; else byte loads with the
//      source index clamped into the frame - which IS the edge replication),
//   2. one thread per 2 x 2 pixels: Y - 128 of the four, Cb - 128 / Cr - 128 of their mean, written in block layout [mcu][6][8][8] fp32,
//   3. one thread per block row: 8-point DCT in place,   4. one thread per block column: 8-point DCT, / q, round half away, -> int16
//      at its zigzag position in LDS,   5. the strip's blocks leave as 16-byte stores (a block = one 128-byte row).
// fp32 throughout, nothing rounded before step 4.  The +128 of Cb / Cr and the level shift cancel and are never added.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kThreads = 256;
constexpr int kChunkMcus = 16;                          // 16 rows x 256 px x 3 B = 12 KiB staged, 96 blocks x 256 B = 24 KiB fp32
constexpr int kChunkPx = kChunkMcus * 16;
constexpr int kChunkBlocks = kChunkMcus * 6;

struct qtabs_t { uint8_t q[128]; };                     // luma [64] | chroma [64], natural (row-major) order

SDV_DEVICE void dct8(const float* in, float* out) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        float s = kDct[u * 8] * in[0];
#pragma unroll
        for (int x = 1; x < 8; ++x) s = __builtin_fmaf(kDct[u * 8 + x], in[x], s);
        out[u] = s;
    }
}

__global__ __launch_bounds__(kThreads) void jpeg_transform_kernel(const uint8_t* __restrict__ frames, int16_t* __restrict__ coef, int H, int W,
                                                                  int mcu_cols, int vec, qtabs_t qt) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[16 * kChunkPx * 3];            // step 1; reused as the int16 output of step 4
    __shared__ __attribute__((aligned(16))) float blk[kChunkBlocks * 64];
    __shared__ float qf[128];
    const int tid = threadIdx.x;
    const int m0 = blockIdx.x * kChunkMcus, r = blockIdx.y, f = blockIdx.z;
    const int nm = min(kChunkMcus, mcu_cols - m0);      // MCUs of this chunk
    const int cw = nm * 16, px0 = m0 * 16, y0 = r * 16;
    const uint8_t* img = frames + (long long)f * H * W * 3;
    if (tid < 128) qf[tid] = (float)qt.q[tid];
    if (vec) {                                          // W % 16 == 0: no column to replicate, cw * 3 bytes = 3 * nm 16-byte pieces per row
        const int nv = nm * 3;
        for (int i = tid; i < 16 * nv; i += kThreads) {
            const int row = i / nv, v = i - row * nv;
            const int ys = min(y0 + row, H - 1);
            *(uint4*)(raw + row * (kChunkPx * 3) + v * 16) = *(const uint4*)(img + ((long long)ys * W + px0) * 3 + v * 16);
        }
    } else {
        const int rb = cw * 3;
        for (int i = tid; i < 16 * rb; i += kThreads) {
            const int row = i / rb, rem = i - row * rb;
            const int x = rem / 3, c = rem - x * 3;
            const int ys = min(y0 + row, H - 1), xs = min(px0 + x, W - 1);
            raw[row * (kChunkPx * 3) + rem] = img[((long long)ys * W + xs) * 3 + c];
        }
    }
    __syncthreads();
    const int qw = cw / 2;
    for (int q = tid; q < 8 * qw; q += kThreads) {
        const int qy = q / qw, qx = q - qy * qw;
        float rs = 0.f, gs = 0.f, bs = 0.f;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int y = 2 * qy + (d >> 1), x = 2 * qx + (d & 1);
            const uint8_t* p = raw + y * (kChunkPx * 3) + x * 3;
            const float R = (float)p[0], G = (float)p[1], B = (float)p[2];
            rs += R, gs += G, bs += B;                  // (sums of four bytes: exact)
            const float Y = __builtin_fmaf(0.114f, B, __builtin_fmaf(0.587f, G, __builtin_fmaf(0.299f, R, -128.0f)));
            const int k = (y >> 3) * 2 + ((x >> 3) & 1);
            blk[((x >> 4) * 6 + k) * 64 + (y & 7) * 8 + (x & 7)] = Y;
        }
        const float cb = __builtin_fmaf(0.5f, bs, __builtin_fmaf(-0.331264108f, gs, -0.168735892f * rs)) * 0.25f;
        const float cr = __builtin_fmaf(-0.081312411f, bs, __builtin_fmaf(-0.418687589f, gs, 0.5f * rs)) * 0.25f;
        const int c0 = ((qx >> 3) * 6 + 4) * 64 + qy * 8 + (qx & 7);
        blk[c0] = cb;
        blk[c0 + 64] = cr;
    }
    __syncthreads();
    const int nb = nm * 6;
    for (int t = tid; t < nb * 8; t += kThreads) {      // rows: 8 consecutive floats, owned by this thread alone
        float in[8], out[8];
        const f32x4_t a = *(const f32x4_t*)(blk + t * 8), b = *(const f32x4_t*)(blk + t * 8 + 4);
        in[0] = a[0], in[1] = a[1], in[2] = a[2], in[3] = a[3], in[4] = b[0], in[5] = b[1], in[6] = b[2], in[7] = b[3];
        dct8(in, out);
        *(f32x4_t*)(blk + t * 8) = f32x4_t{out[0], out[1], out[2], out[3]};
        *(f32x4_t*)(blk + t * 8 + 4) = f32x4_t{out[4], out[5], out[6], out[7]};
    }
    __syncthreads();
    int16_t* o16 = (int16_t*)raw;                       // 96 blocks x 128 B = 12 KiB = the staging buffer, dead since step 2
    for (int t = tid; t < nb * 8; t += kThreads) {
        const int b = t >> 3, c = t & 7;
        const float* q = qf + ((b % 6) < 4 ? 0 : 64);
        float in[8], out[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) in[y] = blk[b * 64 + y * 8 + c];
        dct8(in, out);
#pragma unroll
        for (int v = 0; v < 8; ++v) o16[b * 64 + kZigzagPos[v * 8 + c]] = (int16_t)(int)roundf(out[v] / q[v * 8 + c]);
    }
    __syncthreads();
    int16_t* dst = coef + ((((long long)f * gridDim.y + r) * mcu_cols + m0) * 6) * 64;
    for (int i = tid; i < nb * 8; i += kThreads) ((uint4*)dst)[i] = ((const uint4*)o16)[i];
}

// ---------------------------------------------------------------------------------------------------------------------------
// Entropy coding.  One workgroup = one wave = one restart interval (one MCU row of one frame); lane = block, 64 blocks per pass.
// A pass:  every lane walks its block once for the LENGTH of its bit string, the wave takes the exclusive prefix sum, every lane walks
// the block again and ORs its bits into the pass's bit buffer in LDS (LDS atomic OR: neighbours share a word); then the whole bytes
// of the buffer are byte-stuffed (ballot of the 0xFF lanes + prefix count) and leave; the up to 7 bits left over open the next pass.
// The kernel runs twice: COUNT (WRITE = false) stores only the interval's byte length, the scan below turns lengths into positions,
// WRITE = true stores the bytes at their final place in `out` - there is no per-interval slot that adversarial input could overrun,
// and no store is issued at or beyond out_cap.
// A block's bit string is at most 20 (DC: 9-bit code + 11 bits) + 63 * 26 (AC: 16-bit code + 10 bits) = 1658 bits: size categories
// are clamped to 11 / 10, which a coefficient buffer written by the transform kernel never needs (|DC diff| <= 2044, |AC| <= 1020).
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kMaxBlockBits = 20 + 63 * 26;
constexpr int kBitWords = (64 * kMaxBlockBits + 7 + 31) / 32 + 2;

SDV_DEVICE int size_category(int v) { return 32 - __clz(v < 0 ? -v : v); }       // 0 for v == 0

struct bit_counter {
    unsigned n = 0;
    SDV_DEVICE void put(unsigned, int len) { n += (unsigned)len; }
};
struct bit_writer {                                     // bits [pos, ...) of the LDS buffer, big-endian inside 32-bit words
    unsigned* buf;
    unsigned word;
    int n;
    unsigned long long acc = 0;
    SDV_DEVICE bit_writer(unsigned* b, unsigned pos) : buf(b), word(pos >> 5), n((int)(pos & 31)) {}
    SDV_DEVICE void put(unsigned v, int len) {          // len <= 26, n < 32
        acc |= (unsigned long long)v << (64 - n - len);
        n += len;
        if (n >= 32) {
            atomicOr(buf + word, (unsigned)(acc >> 32));
            ++word;
            acc <<= 32;
            n -= 32;
        }
    }
    SDV_DEVICE void flush() {
        if (n > 0) atomicOr(buf + word, (unsigned)(acc >> 32));
    }
};

template <class Sink>
SDV_DEVICE void code_block(const int16_t* __restrict__ blk, int pred, const unsigned* __restrict__ huff, bool chroma, Sink& sink) {
    const unsigned* dc = huff + (chroma ? kDcChroma : kDcLuma);
    const unsigned* ac = huff + (chroma ? kAcChroma : kAcLuma);
    int run = 0;
#pragma unroll 1
    for (int g = 0; g < 8; ++g) {
        const uint4 raw = ((const uint4*)blk)[g];
        const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int v = (int)(int16_t)(w[e >> 1] >> ((e & 1) * 16));
            if (g == 0 && e == 0) {
                v = min(max(v - pred, -2047), 2047);
                const int s = size_category(v);
                const unsigned h = dc[s];
                sink.put(((h & 0xffffu) << s) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1u)), (int)(h >> 16) + s);
                continue;
            }
            if (v == 0) {
                ++run;
                continue;
            }
            v = min(max(v, -1023), 1023);
            while (run > 15) {
                const unsigned z = ac[0xF0];
                sink.put(z & 0xffffu, (int)(z >> 16));
                run -= 16;
            }
            const int s = size_category(v);
            const unsigned h = ac[(run << 4) | s];
            sink.put(((h & 0xffffu) << s) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1u)), (int)(h >> 16) + s);
            run = 0;
        }
    }
    if (run > 0) {
        const unsigned z = ac[0x00];
        sink.put(z & 0xffffu, (int)(z >> 16));
    }
}

SDV_DEVICE void put_byte(uint8_t* out, long long cap, long long at, unsigned v) {
    if (at < cap) out[at] = (uint8_t)v;
}

template <bool WRITE>
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, int mcu_rows, int mcu_cols, int32_t* __restrict__ lens,
                                                          const long long* __restrict__ starts, const uint8_t* __restrict__ header,
                                                          int header_len, uint8_t* __restrict__ out, long long out_cap,
                                                          const long long* __restrict__ needed) {
    __shared__ unsigned bits[kBitWords];
    __shared__ unsigned huff[kHuffWords];
    const int lane = threadIdx.x;
    const long long interval = blockIdx.x;
    const int row = (int)(interval % mcu_rows);
    long long at = 0;                                   // WRITE: where the next byte of this interval goes
    if (WRITE) {
        if (*needed > out_cap) return;                  // the host retries with a buffer of *needed bytes: nothing is written
        at = starts[interval];
        if (row == 0)
            for (int i = lane; i < header_len; i += 64) put_byte(out, out_cap, at - header_len + i, header[i]);
    }
    for (int i = lane; i < kHuffWords; i += 64) huff[i] = kHuff[i];
    for (int i = lane; i < kBitWords; i += 64) bits[i] = 0u;
    __syncthreads();
    const int nblk = mcu_cols * 6;
    const int16_t* base = coef + interval * nblk * 64;
    unsigned carry = 0;                                 // bits (0..7) of the pass buffer that belong to the previous pass
    long long total = 0;                                // bytes of the interval so far, stuffing included
    for (int b0 = 0; b0 < nblk; b0 += 64) {
        const int b = b0 + lane;
        const bool valid = b < nblk;
        const int k = b % 6, mcu = b / 6;
        const bool chroma = k >= 4;
        int pred = 0;
        unsigned len = 0;
        if (valid) {
            // the previous block of the same component inside the interval: Y follows Y (across the MCU border: Y11 of the MCU before)
            const int prev = chroma ? (mcu > 0 ? b - 6 : -1) : (k > 0 ? b - 1 : (mcu > 0 ? b - 3 : -1));
            if (prev >= 0) pred = base[(long long)prev * 64];
            bit_counter cnt;
            code_block(base + (long long)b * 64, pred, huff, chroma, cnt);
            len = cnt.n;
        }
        unsigned incl = len;                            // wave-wide inclusive prefix sum of the lengths
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        const unsigned pass_bits = carry + __shfl(incl, 63);
        if (valid) {
            bit_writer wr(bits, carry + incl - len);
            code_block(base + (long long)b * 64, pred, huff, chroma, wr);
            wr.flush();
        }
        __syncthreads();
        const unsigned nbytes = pass_bits >> 3;         // whole bytes of this pass
        for (unsigned j0 = 0; j0 < nbytes; j0 += 64) {
            const unsigned j = j0 + lane;
            const bool have = j < nbytes;
            const unsigned byte = have ? (bits[j >> 2] >> (24 - 8 * (j & 3))) & 0xffu : 0u;
            const unsigned long long ff = __ballot(have && byte == 0xffu);
            if (WRITE && have) {
                const long long p = at + total + (j - j0) + __popcll(ff & ((1ull << lane) - 1ull));
                put_byte(out, out_cap, p, byte);
                if (byte == 0xffu) put_byte(out, out_cap, p + 1, 0u);
            }
            total += min(64u, nbytes - j0) + __popcll(ff);
        }
        // the pass's last, partial byte opens the next pass; everything else of the buffer is cleared
        carry = pass_bits & 7u;
        const unsigned last = carry ? (bits[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 0xffu : 0u;
        __syncthreads();
        for (unsigned i = lane; i <= (pass_bits >> 5) + 1 && i < (unsigned)kBitWords; i += 64) bits[i] = i == 0 ? last << 24 : 0u;
        __syncthreads();
    }
    if (carry) {                                        // pad the interval to a byte with 1-bits
        const unsigned byte = (bits[0] >> 24) | ((1u << (8 - carry)) - 1u);
        if (WRITE && lane == 0) {
            put_byte(out, out_cap, at + total, byte);
            if (byte == 0xffu) put_byte(out, out_cap, at + total + 1, 0u);
        }
        total += byte == 0xffu ? 2 : 1;
    }
    if (lane == 0) {
        if (WRITE) {                                    // RSTm between the intervals of a frame (m cycles 0..7), EOI behind the last
            put_byte(out, out_cap, at + total, 0xffu);
            put_byte(out, out_cap, at + total + 1, row == mcu_rows - 1 ? 0xd9u : 0xd0u + (unsigned)(row & 7));
        } else {
            lens[interval] = (int32_t)total;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Scan.  ONE workgroup: exclusive scan of (length + 2 marker bytes) over all intervals, frame-major, plus the header in front of every
// frame -> starts[interval] (first entropy-coded byte), offsets[frame], offsets[n] = *needed = the bytes the whole batch takes.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void jpeg_scan_kernel(const int32_t* __restrict__ lens, long long* __restrict__ starts, long long n_int,
                                                             int mcu_rows, int header_len, long long* __restrict__ offsets,
                                                             long long* __restrict__ needed) {
    __shared__ long long wsum[kThreads / 64];
    __shared__ long long running;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) running = 0;
    __syncthreads();
    for (long long i0 = 0; i0 < n_int; i0 += kThreads) {
        const long long i = i0 + tid;
        const long long mine = i < n_int ? (long long)lens[i] + 2 : 0;
        long long incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        long long before = running;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (i < n_int) {
            const long long f = i / mcu_rows;
            const long long first = before + incl - mine + f * header_len;       // where this interval's part of the file begins
            starts[i] = first + header_len;
            if (i % mcu_rows == 0) offsets[f] = first;
        }
        __syncthreads();
        if (tid == kThreads - 1) running = before + incl;
        __syncthreads();
    }
    if (tid == 0) {
        const long long total = running + (n_int / mcu_rows) * header_len;
        offsets[n_int / mcu_rows] = total;
        *needed = total;
    }
}

}  // namespace

extern "C" int sdv_jpeg_transform_u8(const uint8_t* frames, int32_t n, int32_t H, int32_t W, const uint16_t* qtab_luma,
                                     const uint16_t* qtab_chroma, int16_t* coef, void* stream) {
    SDV_REQUIRE(frames && qtab_luma && qtab_chroma && coef, "sdv_jpeg_transform_u8: null pointer");
    SDV_REQUIRE(n > 0 && n <= 65535, "sdv_jpeg_transform_u8: bad frame count n=%d (1 .. 65535)", n);
    SDV_REQUIRE(H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "sdv_jpeg_transform_u8: bad frame size H=%d W=%d (1 .. 65535)", H, W);
    SDV_REQUIRE((((uintptr_t)coef) & 15) == 0, "sdv_jpeg_transform_u8: coef must be 16-byte aligned (16-byte block stores)");
    qtabs_t qt;
    for (int i = 0; i < 64; ++i) {
        SDV_REQUIRE(qtab_luma[i] >= 1 && qtab_luma[i] <= 255 && qtab_chroma[i] >= 1 && qtab_chroma[i] <= 255,
                    "sdv_jpeg_transform_u8: quantisation table entry %d outside 1 .. 255 (%d / %d)", i, (int)qtab_luma[i], (int)qtab_chroma[i]);
        qt.q[i] = (uint8_t)qtab_luma[i];
        qt.q[64 + i] = (uint8_t)qtab_chroma[i];
    }
    const int mcu_rows = (H + 15) / 16, mcu_cols = (W + 15) / 16;
    const int vec = W % 16 == 0 && (((uintptr_t)frames) & 15) == 0;
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)((mcu_cols + kChunkMcus - 1) / kChunkMcus), (unsigned)mcu_rows, (unsigned)n),
                       dim3(kThreads), 0, (hipStream_t)stream, frames, coef, H, W, mcu_cols, vec, qt);
    SDV_CHECK_LAUNCH("sdv_jpeg_transform_u8");
    return SDV_OK;
}

extern "C" int sdv_jpeg_entropy_pack(const int16_t* coef, int32_t n, int32_t H, int32_t W, const uint8_t* header, int32_t header_len,
                                     void* scratch, int64_t scratch_bytes, uint8_t* out, int64_t out_cap, int64_t* offsets, int64_t* needed,
                                     void* stream) {
    SDV_REQUIRE(coef && header && scratch && out && offsets && needed, "sdv_jpeg_entropy_pack: null pointer");
    SDV_REQUIRE(n > 0 && n <= 65535, "sdv_jpeg_entropy_pack: bad frame count n=%d (1 .. 65535)", n);
    SDV_REQUIRE(H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "sdv_jpeg_entropy_pack: bad frame size H=%d W=%d (1 .. 65535)", H, W);
    SDV_REQUIRE(header_len > 0 && header_len <= 4096, "sdv_jpeg_entropy_pack: bad header length %d (1 .. 4096)", header_len);
    SDV_REQUIRE(out_cap >= 0, "sdv_jpeg_entropy_pack: negative output capacity");
    const int mcu_rows = (H + 15) / 16, mcu_cols = (W + 15) / 16;
    const long long n_int = (long long)n * mcu_rows;
    SDV_REQUIRE(n_int < 0x7fffffffLL, "sdv_jpeg_entropy_pack: too many restart intervals for one grid");
    SDV_REQUIRE(scratch_bytes >= 12 * n_int, "sdv_jpeg_entropy_pack: scratch buffer too small: %lld bytes, %lld restart intervals need %lld",
                (long long)scratch_bytes, n_int, 12 * n_int);
    SDV_REQUIRE((((uintptr_t)coef) & 15) == 0 && (((uintptr_t)scratch) & 7) == 0 && (((uintptr_t)offsets) & 7) == 0 && (((uintptr_t)needed) & 7) == 0,
                "sdv_jpeg_entropy_pack: coef must be 16-byte, scratch / offsets / needed 8-byte aligned");
    long long* starts = (long long*)scratch;            // [n_int] int64, then the lengths [n_int] int32
    int32_t* lens = (int32_t*)(starts + n_int);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3((unsigned)n_int), dim3(64), 0, s, coef, mcu_rows, mcu_cols, lens, (const long long*)starts,
                       header, header_len, out, (long long)out_cap, (const long long*)needed);
    SDV_CHECK_LAUNCH("sdv_jpeg_entropy_pack (count)");
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(kThreads), 0, s, (const int32_t*)lens, starts, n_int, mcu_rows, header_len,
                       (long long*)offsets, (long long*)needed);
    SDV_CHECK_LAUNCH("sdv_jpeg_entropy_pack (scan)");
    hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3((unsigned)n_int), dim3(64), 0, s, coef, mcu_rows, mcu_cols, lens, (const long long*)starts,
                       header, header_len, out, (long long)out_cap, (const long long*)needed);
    SDV_CHECK_LAUNCH("sdv_jpeg_entropy_pack (write)");
    return SDV_OK;
}
