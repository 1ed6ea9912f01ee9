// H.264 CAVLC intra encoder, the part that is plain C++ (sdv_hip.h "H.264 CAVLC intra encoder"): VLC tables, bit writer with emulation
// prevention, transforms, quantisation, residual_block_cavlc(), and the macroblock step of a slice's chain.  Host and device compile the
// same functions: the kernel in sdv_h264.hip walks a slice with them, the host-only table entry point reads the same words.
#pragma once
#include <stdint.h>

// Tables 9-5, 9-7, 9-8, 9-9, 9-10 as (length << 8 | code) words; length 0 = no such symbol.
#define SDV_H264_VLC_WORDS \
    0x0101, 0x0000, 0x0000, 0x0000, 0x0605, 0x0201, 0x0000, 0x0000, 0x0807, 0x0604, 0x0301, 0x0000, 0x0907, 0x0806, 0x0705, 0x0503, \
    0x0a07, 0x0906, 0x0805, 0x0603, 0x0b07, 0x0a06, 0x0905, 0x0704, 0x0d0f, 0x0b06, 0x0a05, 0x0804, 0x0d0b, 0x0d0e, 0x0b05, 0x0904, \
    0x0d08, 0x0d0a, 0x0d0d, 0x0a04, 0x0e0f, 0x0e0e, 0x0d09, 0x0b04, 0x0e0b, 0x0e0a, 0x0e0d, 0x0d0c, 0x0f0f, 0x0f0e, 0x0e09, 0x0e0c, \
    0x0f0b, 0x0f0a, 0x0f0d, 0x0e08, 0x100f, 0x0f01, 0x0f09, 0x0f0c, 0x100b, 0x100e, 0x100d, 0x0f08, 0x1007, 0x100a, 0x1009, 0x100c, \
    0x1004, 0x1006, 0x1005, 0x1008, 0x0203, 0x0000, 0x0000, 0x0000, 0x060b, 0x0202, 0x0000, 0x0000, 0x0607, 0x0507, 0x0303, 0x0000, \
    0x0707, 0x060a, 0x0609, 0x0405, 0x0807, 0x0606, 0x0605, 0x0404, 0x0804, 0x0706, 0x0705, 0x0506, 0x0907, 0x0806, 0x0805, 0x0608, \
    0x0b0f, 0x0906, 0x0905, 0x0604, 0x0b0b, 0x0b0e, 0x0b0d, 0x0704, 0x0c0f, 0x0b0a, 0x0b09, 0x0904, 0x0c0b, 0x0c0e, 0x0c0d, 0x0b0c, \
    0x0c08, 0x0c0a, 0x0c09, 0x0b08, 0x0d0f, 0x0d0e, 0x0d0d, 0x0c0c, 0x0d0b, 0x0d0a, 0x0d09, 0x0d0c, 0x0d07, 0x0e0b, 0x0d06, 0x0d08, \
    0x0e09, 0x0e08, 0x0e0a, 0x0d01, 0x0e07, 0x0e06, 0x0e05, 0x0e04, 0x040f, 0x0000, 0x0000, 0x0000, 0x060f, 0x040e, 0x0000, 0x0000, \
    0x060b, 0x050f, 0x040d, 0x0000, 0x0608, 0x050c, 0x050e, 0x040c, 0x070f, 0x050a, 0x050b, 0x040b, 0x070b, 0x0508, 0x0509, 0x040a, \
    0x0709, 0x060e, 0x060d, 0x0409, 0x0708, 0x060a, 0x0609, 0x0408, 0x080f, 0x070e, 0x070d, 0x050d, 0x080b, 0x080e, 0x070a, 0x060c, \
    0x090f, 0x080a, 0x080d, 0x070c, 0x090b, 0x090e, 0x0809, 0x080c, 0x0908, 0x090a, 0x090d, 0x0808, 0x0a0d, 0x0907, 0x0909, 0x090c, \
    0x0a09, 0x0a0c, 0x0a0b, 0x0a0a, 0x0a05, 0x0a08, 0x0a07, 0x0a06, 0x0a01, 0x0a04, 0x0a03, 0x0a02, 0x0603, 0x0000, 0x0000, 0x0000, \
    0x0600, 0x0601, 0x0000, 0x0000, 0x0604, 0x0605, 0x0606, 0x0000, 0x0608, 0x0609, 0x060a, 0x060b, 0x060c, 0x060d, 0x060e, 0x060f, \
    0x0610, 0x0611, 0x0612, 0x0613, 0x0614, 0x0615, 0x0616, 0x0617, 0x0618, 0x0619, 0x061a, 0x061b, 0x061c, 0x061d, 0x061e, 0x061f, \
    0x0620, 0x0621, 0x0622, 0x0623, 0x0624, 0x0625, 0x0626, 0x0627, 0x0628, 0x0629, 0x062a, 0x062b, 0x062c, 0x062d, 0x062e, 0x062f, \
    0x0630, 0x0631, 0x0632, 0x0633, 0x0634, 0x0635, 0x0636, 0x0637, 0x0638, 0x0639, 0x063a, 0x063b, 0x063c, 0x063d, 0x063e, 0x063f, \
    0x0201, 0x0000, 0x0000, 0x0000, 0x0607, 0x0101, 0x0000, 0x0000, 0x0604, 0x0606, 0x0301, 0x0000, 0x0603, 0x0703, 0x0702, 0x0605, \
    0x0602, 0x0803, 0x0802, 0x0700, 0x0101, 0x0303, 0x0302, 0x0403, 0x0402, 0x0503, 0x0502, 0x0603, 0x0602, 0x0703, 0x0702, 0x0803, \
    0x0802, 0x0903, 0x0902, 0x0901, 0x0307, 0x0306, 0x0305, 0x0304, 0x0303, 0x0405, 0x0404, 0x0403, 0x0402, 0x0503, 0x0502, 0x0603, \
    0x0602, 0x0601, 0x0600, 0x0000, 0x0405, 0x0307, 0x0306, 0x0305, 0x0404, 0x0403, 0x0304, 0x0303, 0x0402, 0x0503, 0x0502, 0x0601, \
    0x0501, 0x0600, 0x0000, 0x0000, 0x0503, 0x0307, 0x0405, 0x0404, 0x0306, 0x0305, 0x0304, 0x0403, 0x0303, 0x0402, 0x0502, 0x0501, \
    0x0500, 0x0000, 0x0000, 0x0000, 0x0405, 0x0404, 0x0403, 0x0307, 0x0306, 0x0305, 0x0304, 0x0303, 0x0402, 0x0501, 0x0401, 0x0500, \
    0x0000, 0x0000, 0x0000, 0x0000, 0x0601, 0x0501, 0x0307, 0x0306, 0x0305, 0x0304, 0x0303, 0x0302, 0x0401, 0x0301, 0x0600, 0x0000, \
    0x0000, 0x0000, 0x0000, 0x0000, 0x0601, 0x0501, 0x0305, 0x0304, 0x0303, 0x0203, 0x0302, 0x0401, 0x0301, 0x0600, 0x0000, 0x0000, \
    0x0000, 0x0000, 0x0000, 0x0000, 0x0601, 0x0401, 0x0501, 0x0303, 0x0203, 0x0202, 0x0302, 0x0301, 0x0600, 0x0000, 0x0000, 0x0000, \
    0x0000, 0x0000, 0x0000, 0x0000, 0x0601, 0x0600, 0x0401, 0x0203, 0x0202, 0x0301, 0x0201, 0x0501, 0x0000, 0x0000, 0x0000, 0x0000, \
    0x0000, 0x0000, 0x0000, 0x0000, 0x0501, 0x0500, 0x0301, 0x0203, 0x0202, 0x0201, 0x0401, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, \
    0x0000, 0x0000, 0x0000, 0x0000, 0x0400, 0x0401, 0x0301, 0x0302, 0x0101, 0x0303, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, \
    0x0000, 0x0000, 0x0000, 0x0000, 0x0400, 0x0401, 0x0201, 0x0101, 0x0301, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, \
    0x0000, 0x0000, 0x0000, 0x0000, 0x0300, 0x0301, 0x0101, 0x0201, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, \
    0x0000, 0x0000, 0x0000, 0x0000, 0x0200, 0x0201, 0x0101, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, \
    0x0000, 0x0000, 0x0000, 0x0000, 0x0100, 0x0101, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, \
    0x0000, 0x0000, 0x0000, 0x0000, 0x0101, 0x0201, 0x0301, 0x0300, 0x0101, 0x0201, 0x0200, 0x0000, 0x0101, 0x0100, 0x0000, 0x0000, \
    0x0101, 0x0100, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, \
    0x0101, 0x0201, 0x0200, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, \
    0x0203, 0x0202, 0x0201, 0x0200, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, \
    0x0203, 0x0202, 0x0201, 0x0301, 0x0300, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, \
    0x0203, 0x0202, 0x0303, 0x0302, 0x0301, 0x0300, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, \
    0x0203, 0x0300, 0x0301, 0x0303, 0x0302, 0x0305, 0x0304, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, \
    0x0307, 0x0306, 0x0305, 0x0304, 0x0303, 0x0302, 0x0301, 0x0401, 0x0501, 0x0601, 0x0701, 0x0801, 0x0901, 0x0a01, 0x0b01, 0x0000

// Offsets into the table above.  coeff_token: [table][4 * TotalCoeff + TrailingOnes], tables nC 0-1 | 2-3 | 4-7 | 8+ (68 words each), then
// chroma DC (20 words); total_zeros: [TotalCoeff - 1][total_zeros] (16 words a row), chroma DC (4 words a row); run_before:
// [min(zerosLeft, 7) - 1][run_before] (16 words a row).
enum { kH264CoeffToken = 0, kH264CoeffTokenChromaDc = 272, kH264TotalZeros = 292, kH264TotalZerosChromaDc = 532, kH264RunBefore = 544,
       kH264VlcWords = 656 };

static const uint16_t kH264VlcHost[kH264VlcWords] = {SDV_H264_VLC_WORDS};
#ifdef __HIPCC__
__constant__ const uint16_t kH264VlcDev[kH264VlcWords] = {SDV_H264_VLC_WORDS};
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SDV_H264_VLC kH264VlcDev
#else
#define SDV_H264_VLC kH264VlcHost
#endif
#ifdef __HIPCC__
#define H264_HD __host__ __device__ inline
#else
#define H264_HD inline
#endif

// MF (forward quantiser) and normAdjust4x4 (8.5.9) by qp % 6 and position class: 0 = both indices even, 1 = both odd, 2 = mixed
H264_HD int h264_mf(int q6, int cls) {
    const int t[18] = {13107, 5243, 8066, 11916, 4660, 7490, 10082, 4194, 6554, 9362, 3647, 5825, 8192, 3355, 5243, 7282, 2893, 4559};
    return t[q6 * 3 + cls];
}
H264_HD int h264_norm(int q6, int cls) {
    const int t[18] = {10, 16, 13, 11, 18, 14, 13, 20, 16, 14, 23, 18, 16, 25, 20, 18, 29, 23};
    return t[q6 * 3 + cls];
}
H264_HD int h264_pos_class(int i, int j) { return ((i | j) & 1) == 0 ? 0 : ((i & j) & 1) ? 1 : 2; }
H264_HD int h264_qpc(int qp) {                          // Table 8-15, chroma_qp_index_offset 0
    const uint8_t t[22] = {29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39};
    return qp < 30 ? qp : t[qp - 30];
}
H264_HD int h264_zigzag(int k) {                        // raster index (row * 4 + column) of scan position k
    const uint8_t t[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
    return t[k];
}
H264_HD int h264_scan_pos(int r) {                      // the inverse: scan position of raster index r
    const uint8_t t[16] = {0, 1, 5, 6, 2, 4, 7, 12, 3, 8, 11, 13, 9, 10, 14, 15};
    return t[r];
}

// The slice's bit stream: MSB first, emulation prevention (7.4.1) applied as the bytes leave, never a store at or beyond cap.
struct h264_writer {
    uint8_t* out;
    long long cap, pos;
    unsigned long long acc;
    int n, zeros;
    long long bits;
    bool failed;
    H264_HD void init(uint8_t* o, long long c) { out = o, cap = c, pos = 0, acc = 0, n = 0, zeros = 0, bits = 0, failed = false; }
    H264_HD void emit(unsigned b) {
        if (zeros >= 2 && b <= 3u) {
            if (pos < cap) out[pos] = 3;
            ++pos;
            zeros = 0;
        }
        if (pos < cap) out[pos] = (uint8_t)b;
        ++pos;
        zeros = b == 0u ? zeros + 1 : 0;
    }
    H264_HD void put(unsigned v, int len) {             // len <= 32
        acc = (acc << len) | v;
        n += len;
        bits += len;
        while (n >= 8) {
            emit((unsigned)(acc >> (n - 8)) & 0xffu);
            n -= 8;
        }
    }
    H264_HD void fail() { failed = true; }
};
struct h264_counter {
    long long bits;
    bool failed;
    H264_HD void put(unsigned, int len) { bits += len; }
    H264_HD void fail() { failed = true; }
};

template <class Sink>
H264_HD void h264_put_ue(Sink& s, unsigned v) {
    int len = 0;
    for (unsigned t = v + 1; t; t >>= 1) ++len;
    s.put(v + 1, 2 * len - 1);
}
template <class Sink>
H264_HD void h264_put_se(Sink& s, int v) { h264_put_ue(s, v > 0 ? (unsigned)(2 * v - 1) : (unsigned)(-2 * v)); }
template <class Sink>
H264_HD void h264_put_vlc(Sink& s, int index) {
    const unsigned w = SDV_H264_VLC[index];
    s.put(w & 0xffu, (int)(w >> 8));
}

// residual_block_cavlc() (7.3.5.3.2, 9.2) of maxc levels in scan order; returns TotalCoeff.  A level that needs level_prefix > 15 marks the
// sink failed (the macroblock is then coded I_PCM).
template <class Sink>
H264_HD int h264_code_block(const int16_t* lv, int maxc, int nC, Sink& s) {
    int idx[16];
    int total = 0;
    for (int i = 0; i < maxc; ++i)
        if (lv[i]) idx[total++] = i;
    int t1 = 0;
    for (int k = total - 1; k >= 0 && t1 < 3; --k) {
        const int v = lv[idx[k]];
        if (v != 1 && v != -1) break;
        ++t1;
    }
    const int table = nC < 0 ? 4 : nC < 2 ? 0 : nC < 4 ? 1 : nC < 8 ? 2 : 3;
    h264_put_vlc(s, kH264CoeffToken + table * 68 + 4 * total + t1);
    if (!total) return 0;
    for (int k = total - 1; k >= total - t1; --k) s.put(lv[idx[k]] < 0 ? 1u : 0u, 1);
    int sl = (total > 10 && t1 < 3) ? 1 : 0;
    for (int k = total - 1 - t1; k >= 0; --k) {
        const int v = lv[idx[k]];
        int lc = v > 0 ? 2 * v - 2 : -2 * v - 1;
        if (k == total - 1 - t1 && t1 < 3) lc -= 2;
        int rest = -1;
        if (sl == 0) {
            if (lc < 14) s.put(1u, lc + 1);
            else if (lc < 30) s.put(1u, 15), s.put((unsigned)(lc - 14), 4);
            else rest = lc - 30;
        } else {
            if (lc < (15 << sl)) s.put(1u, (lc >> sl) + 1), s.put((unsigned)lc & ((1u << sl) - 1u), sl);
            else rest = lc - (15 << sl);
        }
        if (rest >= 0) {
            if (rest >= 4096) s.fail(), rest &= 4095;
            s.put(1u, 16);
            s.put((unsigned)rest, 12);
        }
        if (sl == 0) sl = 1;
        if ((v < 0 ? -v : v) > (3 << (sl - 1)) && sl < 6) ++sl;
    }
    if (total < maxc) {
        const int tz = idx[total - 1] + 1 - total;
        h264_put_vlc(s, maxc == 4 ? kH264TotalZerosChromaDc + (total - 1) * 4 + tz : kH264TotalZeros + (total - 1) * 16 + tz);
        int left = tz;
        for (int k = total - 1; k > 0 && left > 0; --k) {
            const int run = idx[k] - idx[k - 1] - 1;
            h264_put_vlc(s, kH264RunBefore + ((left < 7 ? left : 7) - 1) * 16 + run);
            left -= run;
        }
    }
    return total;
}

H264_HD int h264_nc(int a, int b) {                     // -1 = not available
    if (a >= 0 && b >= 0) return (a + b + 1) >> 1;
    return a >= 0 ? a : b >= 0 ? b : 0;
}

// What a macroblock hands to its right neighbour in the slice: the reconstructed right columns, the AC TotalCoeff of its right blocks.
struct h264_chain {
    int have;
    uint8_t ycol[16], ccol[2][8], tcy[4], tcc[2][2];
};

// Levels of one macroblock in coding order: block 0 Intra16x16DCLevel [16], 1..16 the luma AC blocks by luma4x4BlkIdx [15], 17 / 18 chroma
// DC Cb / Cr [4], 19..26 chroma AC Cb 0..3, Cr 0..3 [15]; 16 int16 each, scan order.
enum { kH264MbBlocks = 27, kH264MbLevels = 27 * 16 };

H264_HD void h264_forward4x4(const int* x, int* w) {    // w = Cf x Cf^T, both [16] raster
    int t[16];
    for (int i = 0; i < 4; ++i) {
        const int a = x[i * 4], b = x[i * 4 + 1], c = x[i * 4 + 2], d = x[i * 4 + 3];
        t[i * 4] = a + b + c + d, t[i * 4 + 1] = 2 * a + b - c - 2 * d, t[i * 4 + 2] = a - b - c + d, t[i * 4 + 3] = a - 2 * b + 2 * c - d;
    }
    for (int j = 0; j < 4; ++j) {
        const int a = t[j], b = t[4 + j], c = t[8 + j], d = t[12 + j];
        w[j] = a + b + c + d, w[4 + j] = 2 * a + b - c - 2 * d, w[8 + j] = a - b - c + d, w[12 + j] = a - 2 * b + 2 * c - d;
    }
}
H264_HD void h264_hadamard4x4(const int* x, int* y) {   // y = H x H, H = [1 1 1 1; 1 1 -1 -1; 1 -1 -1 1; 1 -1 1 -1]
    int t[16];
    for (int i = 0; i < 4; ++i) {
        const int a = x[i * 4], b = x[i * 4 + 1], c = x[i * 4 + 2], d = x[i * 4 + 3];
        t[i * 4] = a + b + c + d, t[i * 4 + 1] = a + b - c - d, t[i * 4 + 2] = a - b - c + d, t[i * 4 + 3] = a - b + c - d;
    }
    for (int j = 0; j < 4; ++j) {
        const int a = t[j], b = t[4 + j], c = t[8 + j], d = t[12 + j];
        y[j] = a + b + c + d, y[4 + j] = a + b - c - d, y[8 + j] = a - b - c + d, y[12 + j] = a - b + c - d;
    }
}
H264_HD void h264_inverse4x4(const int* d, int* r) {    // 8.5.12.2: rows, columns, (x + 32) >> 6
    int f[16];
    for (int i = 0; i < 4; ++i) {
        const int e0 = d[i * 4] + d[i * 4 + 2], e1 = d[i * 4] - d[i * 4 + 2], e2 = (d[i * 4 + 1] >> 1) - d[i * 4 + 3],
                  e3 = d[i * 4 + 1] + (d[i * 4 + 3] >> 1);
        f[i * 4] = e0 + e3, f[i * 4 + 1] = e1 + e2, f[i * 4 + 2] = e1 - e2, f[i * 4 + 3] = e0 - e3;
    }
    for (int j = 0; j < 4; ++j) {
        const int e0 = f[j] + f[8 + j], e1 = f[j] - f[8 + j], e2 = (f[4 + j] >> 1) - f[12 + j], e3 = f[4 + j] + (f[12 + j] >> 1);
        r[j] = (e0 + e3 + 32) >> 6, r[4 + j] = (e1 + e2 + 32) >> 6, r[8 + j] = (e1 - e2 + 32) >> 6, r[12 + j] = (e0 - e3 + 32) >> 6;
    }
}
H264_HD int h264_quant(int w, int mf, int f, int qbits) {
    const long long a = ((long long)(w < 0 ? -w : w) * mf + f) >> qbits;
    return (int)(w < 0 ? -a : a);
}
H264_HD int h264_clip255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// transform + quantise one 4x4 block of (src - pred); AC levels to lv[0..14] in scan order, returns the unquantised DC
H264_HD int h264_block_levels(const uint8_t* src, int stride, int pred, int qp, int16_t* lv, bool* any_ac) {
    int x[16], w[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) x[i * 4 + j] = (int)src[i * stride + j] - pred;
    h264_forward4x4(x, w);
    const int q6 = qp % 6, qbits = 15 + qp / 6, f = (1 << qbits) / 3;
    for (int r = 1; r < 16; ++r) {
        const int l = h264_quant(w[r], h264_mf(q6, h264_pos_class(r >> 2, r & 3)), f, qbits);
        lv[h264_scan_pos(r) - 1] = (int16_t)l;
        if (l) *any_ac = true;
    }
    return w[0];
}
// right column (4 samples) of the reconstruction of one block: AC levels lv[0..14] (scan order), dequantised DC dc
H264_HD void h264_recon_column(const int16_t* lv, int dc, int pred, int qp, uint8_t* col) {
    int d[16], r[16];
    const int q6 = qp % 6, k = qp / 6;
    d[0] = dc;
    for (int p = 1; p < 16; ++p) {
        const int ras = h264_zigzag(p);
        d[ras] = (int)lv[p - 1] * h264_norm(q6, h264_pos_class(ras >> 2, ras & 3)) * (1 << k);
    }
    h264_inverse4x4(d, r);
    for (int i = 0; i < 4; ++i) col[i] = (uint8_t)h264_clip255(pred + r[i * 4 + 3]);
}

// macroblock_layer() of one Intra16x16 macroblock from the levels; returns through the sink.  tcy / tcc receive the AC TotalCoeff.
template <class Sink>
H264_HD void h264_code_mb(const int16_t* lev, int cbp_luma, int cbp_chroma, const h264_chain& left, Sink& s, uint8_t* tcy, uint8_t* tcc) {
    h264_put_ue(s, (unsigned)(1 + 2 + 4 * cbp_chroma + (cbp_luma ? 12 : 0)));
    h264_put_ue(s, 0u);                                 // intra_chroma_pred_mode: DC
    h264_put_se(s, 0);                                  // mb_qp_delta
    for (int i = 0; i < 16; ++i) tcy[i] = 0;            // [by * 4 + bx]
    for (int i = 0; i < 8; ++i) tcc[i] = 0;             // [c * 4 + by * 2 + bx]
    h264_code_block(lev, 16, h264_nc(left.have ? left.tcy[0] : -1, -1), s);
    if (cbp_luma)
        for (int b = 0; b < 16; ++b) {
            const int bx = 2 * ((b >> 2) & 1) + (b & 1), by = 2 * (b >> 3) + ((b >> 1) & 1);
            const int a = bx ? tcy[by * 4 + bx - 1] : left.have ? left.tcy[by] : -1;
            const int t = by ? tcy[(by - 1) * 4 + bx] : -1;
            tcy[by * 4 + bx] = (uint8_t)h264_code_block(lev + (1 + b) * 16, 15, h264_nc(a, t), s);
        }
    if (cbp_chroma)
        for (int c = 0; c < 2; ++c) h264_code_block(lev + (17 + c) * 16, 4, -1, s);
    if (cbp_chroma == 2)
        for (int c = 0; c < 2; ++c)
            for (int b = 0; b < 4; ++b) {
                const int bx = b & 1, by = b >> 1;
                const int a = bx ? tcc[c * 4 + by * 2] : left.have ? left.tcc[c][by] : -1;
                const int t = by ? tcc[c * 4 + bx] : -1;
                tcc[c * 4 + b] = (uint8_t)h264_code_block(lev + (19 + c * 4 + b) * 16, 15, h264_nc(a, t), s);
            }
}

// One macroblock of the chain: sy [16 x 16], sc [2][8 x 8] source samples, lev scratch for kH264MbLevels levels.  Writes the macroblock
// to w, updates the chain.  Returns 1 when it was coded I_PCM.
H264_HD int h264_encode_mb(const uint8_t* sy, const uint8_t* sc, int16_t* lev, h264_chain& ch, int qp, h264_writer& w) {
    const int q6 = qp % 6, qbits = 15 + qp / 6, f = (1 << qbits) / 3;
    int pred_y = 128;
    if (ch.have) {
        int s = 8;
        for (int i = 0; i < 16; ++i) s += ch.ycol[i];
        pred_y = s >> 4;
    }
    for (int i = 0; i < kH264MbLevels; ++i) lev[i] = 0;
    bool any_ac = false;
    int dc[16], hd[16];
    for (int b = 0; b < 16; ++b) {
        const int bx = 2 * ((b >> 2) & 1) + (b & 1), by = 2 * (b >> 3) + ((b >> 1) & 1);
        dc[by * 4 + bx] = h264_block_levels(sy + by * 4 * 16 + bx * 4, 16, pred_y, qp, lev + (1 + b) * 16, &any_ac);
    }
    h264_hadamard4x4(dc, hd);
    for (int r = 0; r < 16; ++r) lev[h264_scan_pos(r)] = (int16_t)h264_quant((hd[r] + 1) >> 1, h264_mf(q6, 0), 2 * f, qbits + 1);
    const int qpc = h264_qpc(qp), c6 = qpc % 6, cbits = 15 + qpc / 6, fc = (1 << cbits) / 3;
    int pred_c[2][2] = {{128, 128}, {128, 128}};        // [component][upper / lower half]
    if (ch.have)
        for (int c = 0; c < 2; ++c)
            for (int h = 0; h < 2; ++h)
                pred_c[c][h] = (ch.ccol[c][4 * h] + ch.ccol[c][4 * h + 1] + ch.ccol[c][4 * h + 2] + ch.ccol[c][4 * h + 3] + 2) >> 2;
    bool any_cac = false, any_cdc = false;
    for (int c = 0; c < 2; ++c) {
        int d2[4];
        for (int b = 0; b < 4; ++b)
            d2[b] = h264_block_levels(sc + c * 64 + (b >> 1) * 4 * 8 + (b & 1) * 4, 8, pred_c[c][b >> 1], qpc, lev + (19 + c * 4 + b) * 16, &any_cac);
        const int y2[4] = {d2[0] + d2[1] + d2[2] + d2[3], d2[0] - d2[1] + d2[2] - d2[3], d2[0] + d2[1] - d2[2] - d2[3], d2[0] - d2[1] - d2[2] + d2[3]};
        for (int i = 0; i < 4; ++i) {
            const int l = h264_quant(y2[i], h264_mf(c6, 0), 2 * fc, cbits + 1);
            lev[(17 + c) * 16 + i] = (int16_t)l;
            if (l) any_cdc = true;
        }
    }
    const int cbp_luma = any_ac ? 15 : 0, cbp_chroma = any_cac ? 2 : any_cdc ? 1 : 0;
    uint8_t tcy[16], tcc[8];
    h264_counter cnt;
    cnt.bits = 0, cnt.failed = false;
    h264_code_mb(lev, cbp_luma, cbp_chroma, ch, cnt, tcy, tcc);
    if (cnt.failed || cnt.bits > 3200) {                // Annex A.3.1 / level_prefix <= 15: I_PCM
        h264_put_ue(w, 25u);
        while (w.n) w.put(0u, 1);                       // pcm_alignment_zero_bit
        for (int i = 0; i < 256; ++i) w.put(sy[i], 8);
        for (int i = 0; i < 128; ++i) w.put(sc[i], 8);
        for (int i = 0; i < 16; ++i) ch.ycol[i] = sy[i * 16 + 15];
        for (int c = 0; c < 2; ++c)
            for (int i = 0; i < 8; ++i) ch.ccol[c][i] = sc[c * 64 + i * 8 + 7];
        for (int i = 0; i < 4; ++i) ch.tcy[i] = 16;
        ch.tcc[0][0] = ch.tcc[0][1] = ch.tcc[1][0] = ch.tcc[1][1] = 16;
        ch.have = 1;
        return 1;
    }
    h264_code_mb(lev, cbp_luma, cbp_chroma, ch, w, tcy, tcc);
    // reconstruction of what the chain reads: the right column of luma blocks (bx = 3) and of chroma blocks (bx = 1)
    int c4[16], fm[16];
    for (int r = 0; r < 16; ++r) c4[r] = lev[h264_scan_pos(r)];
    h264_hadamard4x4(c4, fm);
    const int k = qp / 6, v0 = h264_norm(q6, 0);
    uint8_t ycol[16], ccol[2][8];
    for (int by = 0; by < 4; ++by) {
        const int fv = fm[by * 4 + 3];
        const int dcy = k >= 2 ? fv * v0 * (1 << (k - 2)) : (fv * v0 + (1 << (1 - k))) >> (2 - k);
        const int b = 8 * (by >> 1) + 2 * (by & 1) + 5;  // luma4x4BlkIdx of (bx 3, by): 5, 7, 13, 15
        h264_recon_column(lev + (1 + b) * 16, dcy, pred_y, qp, ycol + 4 * by);
    }
    const int kc = qpc / 6, vc = h264_norm(c6, 0);
    for (int c = 0; c < 2; ++c) {
        const int16_t* d = lev + (17 + c) * 16;
        const int f2[4] = {d[0] + d[1] + d[2] + d[3], d[0] - d[1] + d[2] - d[3], d[0] + d[1] - d[2] - d[3], d[0] - d[1] - d[2] + d[3]};
        for (int by = 0; by < 2; ++by) {
            const int dcc = (f2[by * 2 + 1] * vc * (1 << kc)) >> 1;
            h264_recon_column(lev + (19 + c * 4 + by * 2 + 1) * 16, dcc, pred_c[c][by], qpc, ccol[c] + 4 * by);
        }
    }
    for (int i = 0; i < 16; ++i) ch.ycol[i] = ycol[i];
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 8; ++i) ch.ccol[c][i] = ccol[c][i];
    for (int i = 0; i < 4; ++i) ch.tcy[i] = tcy[i * 4 + 3];
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 2; ++i) ch.tcc[c][i] = tcc[c * 4 + i * 2 + 1];
    ch.have = 1;
    return 0;
}

template <class Sink>
H264_HD void h264_slice_header(Sink& s, unsigned first_mb, unsigned idr_pic_id, int qp, int deblock = 0) {
    h264_put_ue(s, first_mb);
    h264_put_ue(s, 7u);                                 // slice_type: I, and every slice of the picture is
    h264_put_ue(s, 0u);                                 // pic_parameter_set_id
    s.put(0u, 4);                                       // frame_num
    h264_put_ue(s, idr_pic_id);
    s.put(0u, 2);                                       // no_output_of_prior_pics_flag, long_term_reference_flag
    h264_put_se(s, qp - 26);                            // slice_qp_delta against pic_init_qp 26
    if (deblock) {                                      // "H.264 deblocking" (sdv_hip_h264_lf.h): the same three bits
        h264_put_ue(s, 0u);                             // disable_deblocking_filter_idc
        h264_put_se(s, 0), h264_put_se(s, 0);           // slice_alpha_c0_offset_div2, slice_beta_offset_div2
    } else {
        h264_put_ue(s, 1u);                             // disable_deblocking_filter_idc
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// GOP path (sdv_hip.h "H.264 P pictures"): IDR pictures coded as above plus P pictures with zero-motion inter prediction, every sample
// of every macroblock reconstructed.  The macroblock step is cut into per-block pieces (one 4x4 block each: 0..15 luma by
// luma4x4BlkIdx, 16..19 Cb, 20..23 Cr) that the kernel gives one lane each, and serial pieces that one lane runs; h264_gop_encode_mb
// runs them all in order on the host.  Nothing above this line is touched by it.
// ------------------------------------------------------------------------------------------------------------------------------------
enum { kH264ModeIntra = 0, kH264ModeInter = 1, kH264ModeSkip = 2, kH264ModePcm = 3 };
enum { kH264GopMax = 256 };

// coded_block_pattern -> codeNum of me(v), inter column of Table 9-4 (ChromaArrayType 1): the inverse of
// 0 16 1 2 4 8 32 3 5 10 12 15 47 7 11 13 14 6 9 31 35 37 42 44 33 34 36 40 39 43 45 46 17 18 20 24 19 21 26 28 23 27 29 30 22 25 38 41
H264_HD int h264_cbp_inter_code(int cbp) {
    const uint8_t t[48] = {0,  2,  3,  7,  4,  8,  17, 13, 5,  18, 9,  14, 10, 15, 16, 11, 1,  32, 33, 36, 34, 37, 44, 40,
                           35, 45, 38, 41, 39, 42, 43, 19, 6,  24, 25, 20, 26, 21, 46, 28, 27, 47, 22, 29, 23, 30, 31, 12};
    return t[cbp];
}

// The state of one macroblock that the pieces share (LDS in the kernel).
struct __attribute__((aligned(16))) h264_gop_mb {
    uint8_t sy[256], sc[128];                           // source
    uint8_t fy[256], fc[128];                           // reference: the co-located samples of the previous reconstruction (P pictures)
    uint8_t ry[256], rc[128];                           // reconstruction
    int16_t lev[kH264MbLevels];                         // as above; an inter macroblock keeps 16 levels in each of the blocks 1..16
    int dcw[24];                                        // transformed DC of every block (Intra16x16 luma, chroma)
    int dcd[24];                                        // its dequantised DC for the reconstruction
    int pred_y, pred_c[2][2];                           // the DC predictors
    int mode;
};

H264_HD void h264_gop_block_xy(int b, int* x, int* y) {  // sample offset of block b inside its plane of the macroblock
    if (b < 16) *x = 4 * (2 * ((b >> 2) & 1) + (b & 1)), *y = 4 * (2 * (b >> 3) + ((b >> 1) & 1));
    else *x = 4 * (b & 1), *y = 4 * ((b >> 1) & 1);
}

// serial: the DC predictors of the Intra16x16 mode from the chain
H264_HD void h264_gop_pred(h264_gop_mb* mb, const h264_chain& ch) {
    mb->pred_y = 128;
    for (int c = 0; c < 2; ++c) mb->pred_c[c][0] = mb->pred_c[c][1] = 128;
    if (!ch.have) return;
    int s = 8;
    for (int i = 0; i < 16; ++i) s += ch.ycol[i];
    mb->pred_y = s >> 4;
    for (int c = 0; c < 2; ++c)
        for (int h = 0; h < 2; ++h)
            mb->pred_c[c][h] = (ch.ccol[c][4 * h] + ch.ccol[c][4 * h + 1] + ch.ccol[c][4 * h + 2] + ch.ccol[c][4 * h + 3] + 2) >> 2;
}

// per luma block: its part of sad_intra and sad_inter
H264_HD void h264_gop_block_sad(const h264_gop_mb* mb, int b, int* intra, int* inter) {
    int x, y, si = 0, sp = 0;
    h264_gop_block_xy(b, &x, &y);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const int s = mb->sy[(y + i) * 16 + x + j], di = s - mb->pred_y, dp = s - (int)mb->fy[(y + i) * 16 + x + j];
            si += di < 0 ? -di : di, sp += dp < 0 ? -dp : dp;
        }
    *intra = si, *inter = sp;
}

// per block: residual, forward transform, quantisation; returns whether the block has a nonzero level that the cbp looks at (Intra16x16
// luma and all chroma: AC only; inter luma: all 16)
H264_HD bool h264_gop_block_forward(h264_gop_mb* mb, int b, bool inter, int qp) {
    int x, y, xs[16], w[16];
    h264_gop_block_xy(b, &x, &y);
    const bool luma = b < 16;
    const int c = (b - 16) >> 2, stride = luma ? 16 : 8;
    const uint8_t* src = luma ? mb->sy : mb->sc + c * 64;
    const uint8_t* ref = luma ? mb->fy : mb->fc + c * 64;
    const int dc_pred = luma ? mb->pred_y : mb->pred_c[c][y >> 2];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const int at = (y + i) * stride + x + j;
            xs[i * 4 + j] = (int)src[at] - (inter ? (int)ref[at] : dc_pred);
        }
    h264_forward4x4(xs, w);
    const int q = luma ? qp : h264_qpc(qp), q6 = q % 6, qbits = 15 + q / 6, f = (1 << qbits) / (inter ? 6 : 3);
    int16_t* lv = mb->lev + (luma ? 1 + b : 19 + (b - 16)) * 16;
    bool any = false;
    const bool whole = luma && inter;                   // 16 levels, the DC among them
    for (int r = whole ? 0 : 1; r < 16; ++r) {
        const int l = h264_quant(w[r], h264_mf(q6, h264_pos_class(r >> 2, r & 3)), f, qbits);
        lv[h264_scan_pos(r) - (whole ? 0 : 1)] = (int16_t)l;
        if (l) any = true;
    }
    if (!whole) lv[15] = 0;
    mb->dcw[b] = w[0];
    return any;
}

// serial: the DC blocks (Intra16x16 luma Hadamard; chroma 2x2), their levels and their dequantised values; returns whether a chroma DC
// level is nonzero
H264_HD bool h264_gop_dc(h264_gop_mb* mb, bool inter, int qp) {
    const int q6 = qp % 6, qbits = 15 + qp / 6, f = (1 << qbits) / 3, k = qp / 6, v0 = h264_norm(q6, 0);
    if (!inter) {
        int dc[16], hd[16], c4[16], fm[16];
        for (int b = 0; b < 16; ++b) {
            int x, y;
            h264_gop_block_xy(b, &x, &y);
            dc[y + (x >> 2)] = mb->dcw[b];
        }
        h264_hadamard4x4(dc, hd);
        for (int r = 0; r < 16; ++r) {
            c4[r] = h264_quant((hd[r] + 1) >> 1, h264_mf(q6, 0), 2 * f, qbits + 1);
            mb->lev[h264_scan_pos(r)] = (int16_t)c4[r];
        }
        h264_hadamard4x4(c4, fm);
        for (int b = 0; b < 16; ++b) {
            int x, y;
            h264_gop_block_xy(b, &x, &y);
            const int fv = fm[y + (x >> 2)];
            mb->dcd[b] = k >= 2 ? fv * v0 * (1 << (k - 2)) : (fv * v0 + (1 << (1 - k))) >> (2 - k);
        }
    } else {
        for (int i = 0; i < 16; ++i) mb->lev[i] = 0;
    }
    const int qpc = h264_qpc(qp), c6 = qpc % 6, cbits = 15 + qpc / 6, fc = (1 << cbits) / (inter ? 6 : 3), kc = qpc / 6, vc = h264_norm(c6, 0);
    bool any = false;
    for (int c = 0; c < 2; ++c) {
        const int* d2 = mb->dcw + 16 + 4 * c;
        const int y2[4] = {d2[0] + d2[1] + d2[2] + d2[3], d2[0] - d2[1] + d2[2] - d2[3], d2[0] + d2[1] - d2[2] - d2[3], d2[0] - d2[1] - d2[2] + d2[3]};
        int d[4];
        for (int i = 0; i < 4; ++i) {
            d[i] = h264_quant(y2[i], h264_mf(c6, 0), 2 * fc, cbits + 1);
            mb->lev[(17 + c) * 16 + i] = (int16_t)d[i];
            if (d[i]) any = true;
        }
        for (int i = 4; i < 16; ++i) mb->lev[(17 + c) * 16 + i] = 0;
        const int f2[4] = {d[0] + d[1] + d[2] + d[3], d[0] - d[1] + d[2] - d[3], d[0] + d[1] - d[2] - d[3], d[0] - d[1] - d[2] + d[3]};
        for (int i = 0; i < 4; ++i) mb->dcd[16 + 4 * c + i] = (f2[i] * vc * (1 << kc)) >> 1;
    }
    return any;
}

// macroblock_layer() of an Intra16x16 macroblock, mb_type offset 0 in an I slice, 5 in a P slice
template <class Sink>
H264_HD void h264_gop_code_intra(const int16_t* lev, int cbp_luma, int cbp_chroma, const h264_chain& left, int type_offset, Sink& s, uint8_t* tcy,
                                 uint8_t* tcc) {
    h264_put_ue(s, (unsigned)(type_offset + 1 + 2 + 4 * cbp_chroma + (cbp_luma ? 12 : 0)));
    h264_put_ue(s, 0u);                                 // intra_chroma_pred_mode: DC
    h264_put_se(s, 0);                                  // mb_qp_delta
    h264_code_block(lev, 16, h264_nc(left.have ? left.tcy[0] : -1, -1), s);
    if (cbp_luma)
        for (int b = 0; b < 16; ++b) {
            const int bx = 2 * ((b >> 2) & 1) + (b & 1), by = 2 * (b >> 3) + ((b >> 1) & 1);
            const int a = bx ? tcy[by * 4 + bx - 1] : left.have ? left.tcy[by] : -1;
            const int t = by ? tcy[(by - 1) * 4 + bx] : -1;
            tcy[by * 4 + bx] = (uint8_t)h264_code_block(lev + (1 + b) * 16, 15, h264_nc(a, t), s);
        }
}
// macroblock_layer() of a P_L0_16x16 macroblock (cbp != 0) up to and including the luma residual
template <class Sink>
H264_HD void h264_gop_code_inter(const int16_t* lev, int cbp_luma, int cbp_chroma, const h264_chain& left, Sink& s, uint8_t* tcy) {
    h264_put_ue(s, 0u);                                 // mb_type P_L0_16x16 (ref_idx_l0 is not sent: one active reference)
    h264_put_se(s, 0), h264_put_se(s, 0);               // mvd_l0
    h264_put_ue(s, (unsigned)h264_cbp_inter_code(cbp_luma + 16 * cbp_chroma));
    h264_put_se(s, 0);                                  // mb_qp_delta
    for (int b = 0; b < 16; ++b) {
        if (!((cbp_luma >> (b >> 2)) & 1)) continue;
        const int bx = 2 * ((b >> 2) & 1) + (b & 1), by = 2 * (b >> 3) + ((b >> 1) & 1);
        const int a = bx ? tcy[by * 4 + bx - 1] : left.have ? left.tcy[by] : -1;
        const int t = by ? tcy[(by - 1) * 4 + bx] : -1;
        tcy[by * 4 + bx] = (uint8_t)h264_code_block(lev + (1 + b) * 16, 16, h264_nc(a, t), s);
    }
}
// the chroma residual of either
template <class Sink>
H264_HD void h264_gop_code_chroma(const int16_t* lev, int cbp_chroma, const h264_chain& left, Sink& s, uint8_t* tcc) {
    if (cbp_chroma)
        for (int c = 0; c < 2; ++c) h264_code_block(lev + (17 + c) * 16, 4, -1, s);
    if (cbp_chroma == 2)
        for (int c = 0; c < 2; ++c)
            for (int b = 0; b < 4; ++b) {
                const int bx = b & 1, by = b >> 1;
                const int a = bx ? tcc[c * 4 + by * 2] : left.have ? left.tcc[c][by] : -1;
                const int t = by ? tcc[c * 4 + bx] : -1;
                tcc[c * 4 + b] = (uint8_t)h264_code_block(lev + (19 + c * 4 + b) * 16, 15, h264_nc(a, t), s);
            }
}
template <class Sink>
H264_HD void h264_gop_code_mb(const int16_t* lev, bool inter, bool p_slice, int cbp_luma, int cbp_chroma, const h264_chain& left, Sink& s,
                              uint8_t* tcy, uint8_t* tcc) {
    for (int i = 0; i < 16; ++i) tcy[i] = 0;            // [by * 4 + bx]
    for (int i = 0; i < 8; ++i) tcc[i] = 0;             // [c * 4 + by * 2 + bx]
    if (inter) h264_gop_code_inter(lev, cbp_luma, cbp_chroma, left, s, tcy);
    else h264_gop_code_intra(lev, cbp_luma, cbp_chroma, left, p_slice ? 5 : 0, s, tcy, tcc);
    h264_gop_code_chroma(lev, cbp_chroma, left, s, tcc);
}

// serial: mode decision after the levels are known (nz: bit b set when h264_gop_block_forward returned true for block b), the counting
// pass, the I_PCM decision, the bits; leaves mb->mode and the chain's TotalCoeffs.  skip_run: the P_Skip macroblocks not yet written.
H264_HD void h264_gop_serial(h264_gop_mb* mb, unsigned nz, bool any_cdc, bool inter, bool p_slice, h264_chain& ch, h264_writer& w, int* skip_run) {
    int cbp_luma = 0;
    if (inter) {
        for (int i = 0; i < 4; ++i)
            if (nz & (0xfu << (4 * i))) cbp_luma |= 1 << i;
    } else if (nz & 0xffffu) {
        cbp_luma = 15;
    }
    const int cbp_chroma = (nz & 0xff0000u) ? 2 : any_cdc ? 1 : 0;
    if (inter && !cbp_luma && !cbp_chroma) {            // P_Skip: inferred vector (0, 0), no residual
        ++*skip_run;
        mb->mode = kH264ModeSkip;
        for (int i = 0; i < 4; ++i) ch.tcy[i] = 0;
        ch.tcc[0][0] = ch.tcc[0][1] = ch.tcc[1][0] = ch.tcc[1][1] = 0;
        return;
    }
    if (p_slice) {
        h264_put_ue(w, (unsigned)*skip_run);            // mb_skip_run
        *skip_run = 0;
    }
    uint8_t tcy[16], tcc[8];
    h264_counter cnt;
    cnt.bits = 0, cnt.failed = false;
    h264_gop_code_mb(mb->lev, inter, p_slice, cbp_luma, cbp_chroma, ch, cnt, tcy, tcc);
    if (cnt.failed || cnt.bits > 3200) {                // Annex A.3.1 / level_prefix <= 15: I_PCM
        h264_put_ue(w, p_slice ? 30u : 25u);
        while (w.n) w.put(0u, 1);                       // pcm_alignment_zero_bit
        for (int i = 0; i < 256; ++i) w.put(mb->sy[i], 8);
        for (int i = 0; i < 128; ++i) w.put(mb->sc[i], 8);
        for (int i = 0; i < 4; ++i) ch.tcy[i] = 16;
        ch.tcc[0][0] = ch.tcc[0][1] = ch.tcc[1][0] = ch.tcc[1][1] = 16;
        mb->mode = kH264ModePcm;
        return;
    }
    h264_gop_code_mb(mb->lev, inter, p_slice, cbp_luma, cbp_chroma, ch, w, tcy, tcc);
    for (int i = 0; i < 4; ++i) ch.tcy[i] = tcy[i * 4 + 3];
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 2; ++i) ch.tcc[c][i] = tcc[c * 4 + i * 2 + 1];
    mb->mode = inter ? kH264ModeInter : kH264ModeIntra;
}

// per block: reconstruction (8.5) by the macroblock's mode
H264_HD void h264_gop_block_recon(h264_gop_mb* mb, int b, int qp) {
    int x, y;
    h264_gop_block_xy(b, &x, &y);
    const bool luma = b < 16;
    const int c = (b - 16) >> 2, stride = luma ? 16 : 8;
    const uint8_t* src = luma ? mb->sy : mb->sc + c * 64;
    const uint8_t* ref = luma ? mb->fy : mb->fc + c * 64;
    uint8_t* rec = luma ? mb->ry : mb->rc + c * 64;
    const int mode = mb->mode;
    if (mode == kH264ModePcm || mode == kH264ModeSkip) {
        const uint8_t* from = mode == kH264ModePcm ? src : ref;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) rec[(y + i) * stride + x + j] = from[(y + i) * stride + x + j];
        return;
    }
    const bool inter = mode == kH264ModeInter, whole = luma && inter;
    const int q = luma ? qp : h264_qpc(qp), q6 = q % 6, k = q / 6;
    const int16_t* lv = mb->lev + (luma ? 1 + b : 19 + (b - 16)) * 16;
    int d[16], r[16];
    for (int p = whole ? 0 : 1; p < 16; ++p) {
        const int ras = h264_zigzag(p);
        d[ras] = (int)lv[p - (whole ? 0 : 1)] * h264_norm(q6, h264_pos_class(ras >> 2, ras & 3)) * (1 << k);
    }
    if (!whole) d[0] = mb->dcd[b];
    h264_inverse4x4(d, r);
    const int dc_pred = luma ? mb->pred_y : mb->pred_c[c][y >> 2];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const int at = (y + i) * stride + x + j;
            rec[at] = (uint8_t)h264_clip255((inter ? (int)ref[at] : dc_pred) + r[i * 4 + j]);
        }
}

// serial: what the right neighbour reads of the reconstruction
H264_HD void h264_gop_chain(const h264_gop_mb* mb, h264_chain& ch) {
    for (int i = 0; i < 16; ++i) ch.ycol[i] = mb->ry[i * 16 + 15];
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 8; ++i) ch.ccol[c][i] = mb->rc[c * 64 + i * 8 + 7];
    ch.have = 1;
}

// P slice header (7.3.3): frame_num u(4), no override, no list modification, sliding-window marking
template <class Sink>
H264_HD void h264_p_slice_header(Sink& s, unsigned first_mb, unsigned frame_num, int qp, int deblock = 0) {
    h264_put_ue(s, first_mb);
    h264_put_ue(s, 5u);                                 // slice_type: P, and every slice of the picture is
    h264_put_ue(s, 0u);                                 // pic_parameter_set_id
    s.put(frame_num & 15u, 4);
    s.put(0u, 3);                                       // num_ref_idx_active_override_flag, ref_pic_list_modification_flag_l0,
                                                        // adaptive_ref_pic_marking_mode_flag
    h264_put_se(s, qp - 26);
    if (deblock) {                                      // "H.264 deblocking" (sdv_hip_h264_lf.h): the same three bits
        h264_put_ue(s, 0u);                             // disable_deblocking_filter_idc
        h264_put_se(s, 0), h264_put_se(s, 0);           // slice_alpha_c0_offset_div2, slice_beta_offset_div2
    } else {
        h264_put_ue(s, 1u);                             // disable_deblocking_filter_idc
    }
}

// The whole macroblock step in order, one piece after the other (host; the kernel spreads the per-block pieces over its lanes).
// mb->sy / sc (and fy / fc in a P picture) are loaded; leaves mb->ry / rc.
inline void h264_gop_encode_mb(h264_gop_mb* mb, h264_chain& ch, bool p_slice, int qp, h264_writer& w, int* skip_run) {
    h264_gop_pred(mb, ch);
    bool inter = false;
    if (p_slice) {
        int si = 0, sp = 0;
        for (int b = 0; b < 16; ++b) {
            int a, c;
            h264_gop_block_sad(mb, b, &a, &c);
            si += a, sp += c;
        }
        inter = !(si < sp);
    }
    unsigned nz = 0;
    for (int b = 0; b < 24; ++b)
        if (h264_gop_block_forward(mb, b, inter, qp)) nz |= 1u << b;
    const bool any_cdc = h264_gop_dc(mb, inter, qp);
    h264_gop_serial(mb, nz, any_cdc, inter, p_slice, ch, w, skip_run);
    for (int b = 0; b < 24; ++b) h264_gop_block_recon(mb, b, qp);
    h264_gop_chain(mb, ch);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Motion-compensated P pictures (sdv_hip_ext.h "H.264 motion search"): one vector per macroblock, every component a multiple of two luma
// samples, so that luma and chroma predictions are plain displaced copies.  The pieces below are what the search kernel, the per-position
// GOP kernel and the host share; nothing above this line is touched by them.
// ------------------------------------------------------------------------------------------------------------------------------------
enum { kH264SearchMax = 16 };

// lambda(qp) = max(1, round(2 ** ((qp - 12) / 6))): what one bit of a vector costs in units of SAD.  A setting, not a measured optimum.
H264_HD int h264_me_lambda(int qp) {
    const uint8_t t[52] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20,
                           23, 25, 29, 32, 36, 40, 45, 51, 57, 64, 72, 81, 91};
    return t[qp];
}
H264_HD int h264_se_bits(int v) {                       // length of se(v)
    h264_counter c;
    c.bits = 0, c.failed = false;
    h264_put_se(c, v);
    return (int)c.bits;
}
// cost(v) = SAD(v) + lambda * (B(vx) + B(vy)), B(c) the length of se(4 c): the vector against a zero predictor
H264_HD int h264_me_cost(int sad, int lambda, int vx, int vy) { return sad + lambda * (h264_se_bits(4 * vx) + h264_se_bits(4 * vy)); }
// The total order (cost, |vx| + |vy|, vy, vx) as one unsigned word: cost < 2^17, the three tie fields halved and biased into 5 bits each.
H264_HD unsigned h264_me_key(int cost, int vx, int vy) {
    const int a = (vx < 0 ? -vx : vx) + (vy < 0 ? -vy : vy);
    return ((unsigned)cost << 15) | ((unsigned)(a >> 1) << 10) | ((unsigned)((vy + 16) >> 1) << 5) | (unsigned)((vx + 16) >> 1);
}
H264_HD void h264_me_unkey(unsigned key, int* cost, int* vx, int* vy) {
    *cost = (int)(key >> 15), *vy = 2 * (int)((key >> 5) & 31u) - 16, *vx = 2 * (int)(key & 31u) - 16;
}
// A vector the stream rule admits for macroblock (mx, my): even, inside the range, the displaced block wholly inside the padded picture.
H264_HD bool h264_mv_valid(int vx, int vy, int search, int mx, int my, int mbw, int mbh) {
    if ((vx & 1) || (vy & 1) || vx < -search || vx > search || vy < -search || vy > search) return false;
    const int x = 16 * mx + vx, y = 16 * my + vy;
    return x >= 0 && x + 16 <= 16 * mbw && y >= 0 && y + 16 <= 16 * mbh;
}
// Where the prediction of macroblock (mx, my) is fetched from: the vector that is coded (the given one when it is valid, else (0, 0)) and
// the offsets of the displaced block's first luma / chroma sample from the first sample of the reference picture's planes.
struct h264_mv_ref {
    int vx, vy;
    long long yoff, coff;
};
H264_HD h264_mv_ref h264_mv_fetch(int vx, int vy, int search, int mx, int my, int mbw, int mbh) {
    h264_mv_ref r;
    const bool ok = h264_mv_valid(vx, vy, search, mx, my, mbw, mbh);
    r.vx = ok ? vx : 0, r.vy = ok ? vy : 0;
    r.yoff = (16LL * my + r.vy) * (16LL * mbw) + 16LL * mx + r.vx;
    r.coff = (8LL * my + r.vy / 2) * (8LL * mbw) + 8LL * mx + r.vx / 2;
    return r;
}

// What a macroblock hands to its right neighbour for 8.4.1.3 (B, C and D lie in another slice): its vector when it is inter (P_Skip
// counts, with (0, 0)), (0, 0) when it is intra or I_PCM or when there is no left neighbour.  Luma samples.
struct h264_mv_chain {
    int vx, vy;
};

// macroblock_layer() of a P_L0_16x16 macroblock with mvd_l0, up to and including the luma residual; cbp 0 carries no mb_qp_delta
template <class Sink>
H264_HD void h264_gop_code_inter_mv(const int16_t* lev, int cbp_luma, int cbp_chroma, const h264_chain& left, int mvdx, int mvdy, Sink& s, uint8_t* tcy) {
    h264_put_ue(s, 0u);                                 // mb_type P_L0_16x16 (ref_idx_l0 is not sent: one active reference)
    h264_put_se(s, mvdx), h264_put_se(s, mvdy);         // mvd_l0, quarter samples
    h264_put_ue(s, (unsigned)h264_cbp_inter_code(cbp_luma + 16 * cbp_chroma));
    if (cbp_luma || cbp_chroma) h264_put_se(s, 0);      // mb_qp_delta
    for (int b = 0; b < 16; ++b) {
        if (!((cbp_luma >> (b >> 2)) & 1)) continue;
        const int bx = 2 * ((b >> 2) & 1) + (b & 1), by = 2 * (b >> 3) + ((b >> 1) & 1);
        const int a = bx ? tcy[by * 4 + bx - 1] : left.have ? left.tcy[by] : -1;
        const int t = by ? tcy[(by - 1) * 4 + bx] : -1;
        tcy[by * 4 + bx] = (uint8_t)h264_code_block(lev + (1 + b) * 16, 16, h264_nc(a, t), s);
    }
}
template <class Sink>
H264_HD void h264_gop_code_mb_mv(const int16_t* lev, bool inter, bool p_slice, int cbp_luma, int cbp_chroma, const h264_chain& left, int mvdx, int mvdy,
                                 Sink& s, uint8_t* tcy, uint8_t* tcc) {
    for (int i = 0; i < 16; ++i) tcy[i] = 0;            // [by * 4 + bx]
    for (int i = 0; i < 8; ++i) tcc[i] = 0;             // [c * 4 + by * 2 + bx]
    if (inter) h264_gop_code_inter_mv(lev, cbp_luma, cbp_chroma, left, mvdx, mvdy, s, tcy);
    else h264_gop_code_intra(lev, cbp_luma, cbp_chroma, left, p_slice ? 5 : 0, s, tcy, tcc);
    h264_gop_code_chroma(lev, cbp_chroma, left, s, tcc);
}

// serial: h264_gop_serial with the macroblock's vector (vx, vy) (luma samples, already through h264_mv_fetch; mb->fy / fc hold the displaced
// reference).  P_Skip needs cbp 0 and the vector (0, 0); cbp 0 with another vector is P_L0_16x16 with coded_block_pattern codeNum 0.  The
// counting pass includes the mvd bits.  Leaves in mvc what the right neighbour predicts its vector from.
H264_HD void h264_gop_serial_mv(h264_gop_mb* mb, unsigned nz, bool any_cdc, bool inter, bool p_slice, h264_chain& ch, h264_mv_chain& mvc, int vx, int vy,
                                h264_writer& w, int* skip_run) {
    int cbp_luma = 0;
    if (inter) {
        for (int i = 0; i < 4; ++i)
            if (nz & (0xfu << (4 * i))) cbp_luma |= 1 << i;
    } else if (nz & 0xffffu) {
        cbp_luma = 15;
    }
    const int cbp_chroma = (nz & 0xff0000u) ? 2 : any_cdc ? 1 : 0;
    const int mvdx = 4 * (vx - mvc.vx), mvdy = 4 * (vy - mvc.vy);
    if (inter && !cbp_luma && !cbp_chroma && !vx && !vy) {  // P_Skip: inferred vector (0, 0), no residual
        ++*skip_run;
        mb->mode = kH264ModeSkip;
        for (int i = 0; i < 4; ++i) ch.tcy[i] = 0;
        ch.tcc[0][0] = ch.tcc[0][1] = ch.tcc[1][0] = ch.tcc[1][1] = 0;
        mvc.vx = mvc.vy = 0;
        return;
    }
    if (p_slice) {
        h264_put_ue(w, (unsigned)*skip_run);            // mb_skip_run
        *skip_run = 0;
    }
    uint8_t tcy[16], tcc[8];
    h264_counter cnt;
    cnt.bits = 0, cnt.failed = false;
    h264_gop_code_mb_mv(mb->lev, inter, p_slice, cbp_luma, cbp_chroma, ch, mvdx, mvdy, cnt, tcy, tcc);
    if (cnt.failed || cnt.bits > 3200) {                // Annex A.3.1 / level_prefix <= 15: I_PCM
        h264_put_ue(w, p_slice ? 30u : 25u);
        while (w.n) w.put(0u, 1);                       // pcm_alignment_zero_bit
        for (int i = 0; i < 256; ++i) w.put(mb->sy[i], 8);
        for (int i = 0; i < 128; ++i) w.put(mb->sc[i], 8);
        for (int i = 0; i < 4; ++i) ch.tcy[i] = 16;
        ch.tcc[0][0] = ch.tcc[0][1] = ch.tcc[1][0] = ch.tcc[1][1] = 16;
        mb->mode = kH264ModePcm;
        mvc.vx = mvc.vy = 0;
        return;
    }
    h264_gop_code_mb_mv(mb->lev, inter, p_slice, cbp_luma, cbp_chroma, ch, mvdx, mvdy, w, tcy, tcc);
    for (int i = 0; i < 4; ++i) ch.tcy[i] = tcy[i * 4 + 3];
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 2; ++i) ch.tcc[c][i] = tcc[c * 4 + i * 2 + 1];
    mb->mode = inter ? kH264ModeInter : kH264ModeIntra;
    mvc.vx = inter ? vx : 0, mvc.vy = inter ? vy : 0;
}

// h264_gop_encode_mb with a vector: mb->sy / sc are loaded, and in a P picture mb->fy / fc from the position h264_mv_fetch gave for
// (vx, vy); leaves mb->ry / rc.  (Host; the kernel spreads the per-block pieces over its lanes.)
inline void h264_gop_encode_mb_mv(h264_gop_mb* mb, h264_chain& ch, h264_mv_chain& mvc, bool p_slice, int qp, int vx, int vy, h264_writer& w,
                                  int* skip_run) {
    h264_gop_pred(mb, ch);
    bool inter = false;
    if (p_slice) {
        int si = 0, sp = 0;
        for (int b = 0; b < 16; ++b) {
            int a, c;
            h264_gop_block_sad(mb, b, &a, &c);
            si += a, sp += c;
        }
        inter = !(si < sp);
    }
    unsigned nz = 0;
    for (int b = 0; b < 24; ++b)
        if (h264_gop_block_forward(mb, b, inter, qp)) nz |= 1u << b;
    const bool any_cdc = h264_gop_dc(mb, inter, qp);
    h264_gop_serial_mv(mb, nz, any_cdc, inter, p_slice, ch, mvc, vx, vy, w, skip_run);
    for (int b = 0; b < 24; ++b) h264_gop_block_recon(mb, b, qp);
    h264_gop_chain(mb, ch);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Sub-sample motion (sdv_hip_h264_sub.h "H.264 sub-sample motion"): vectors in QUARTER luma samples on a grid of 4 / subpel quarters,
// 6-tap luma (8.4.2.2.1) and bilinear chroma (8.4.2.2.2) prediction.  The two functions below are the only interpolators: the search's
// refinement, the per-position GOP kernel and the host build all read a staged window through them.  Nothing above is touched.
// ------------------------------------------------------------------------------------------------------------------------------------
H264_HD int h264_sub_tap6(const uint8_t* p, int step) {                           // E - 5F + 20G + 20H - 5I + J, p at G
    return (int)p[-2 * step] - 5 * (int)p[-step] + 20 * (int)p[0] + 20 * (int)p[step] - 5 * (int)p[2 * step] + (int)p[3 * step];
}
H264_HD int h264_sub_half(int v1) { return h264_clip255((v1 + 16) >> 5); }
// One luma sample: ``g`` points at the whole sample G of the integer part inside a staged window of row length ``stride`` that holds
// two more samples before and three after G in both directions; (xf, yf) in 0 .. 3 are the quarter fractions.
H264_HD int h264_sub_luma(const uint8_t* g, int stride, int xf, int yf) {
    if (!(xf | yf)) return g[0];
    if (!yf) {                                          // a, b, c
        const int b = h264_sub_half(h264_sub_tap6(g, 1));
        return xf == 2 ? b : ((int)g[xf >> 1] + b + 1) >> 1;
    }
    if (!xf) {                                          // d, h, n
        const int h = h264_sub_half(h264_sub_tap6(g, stride));
        return yf == 2 ? h : ((int)g[(yf >> 1) * stride] + h + 1) >> 1;
    }
    if ((xf & 1) && (yf & 1)) {                         // e, g, p, r: the b-type sample of row yf >> 1 and the h-type sample of column xf >> 1
        const int b = h264_sub_half(h264_sub_tap6(g + (yf >> 1) * stride, 1));
        const int h = h264_sub_half(h264_sub_tap6(g + (xf >> 1), stride));
        return (b + h + 1) >> 1;
    }
    const int j1 = h264_sub_tap6(g - 2 * stride, 1) - 5 * h264_sub_tap6(g - stride, 1) + 20 * h264_sub_tap6(g, 1) +
                   20 * h264_sub_tap6(g + stride, 1) - 5 * h264_sub_tap6(g + 2 * stride, 1) + h264_sub_tap6(g + 3 * stride, 1);
    const int j = h264_clip255((j1 + 512) >> 10);       // j: the 6-tap over the unclipped row intermediates
    if (xf == 2 && yf == 2) return j;
    if (xf == 2) return (h264_sub_half(h264_sub_tap6(g + (yf >> 1) * stride, 1)) + j + 1) >> 1;      // f, q: b or s
    return (h264_sub_half(h264_sub_tap6(g + (xf >> 1), stride)) + j + 1) >> 1;                        // i, k: h or m
}
// One chroma sample: ``a`` points at sample A of the integer part (B right of it, C below, D diagonal); (xf, yf) in 0 .. 7.
H264_HD int h264_sub_chroma(const uint8_t* a, int stride, int xf, int yf) {
    return ((8 - xf) * (8 - yf) * (int)a[0] + xf * (8 - yf) * (int)a[1] + (8 - xf) * yf * (int)a[stride] + xf * yf * (int)a[stride + 1] + 32) >> 6;
}
enum { kH264SubLumaWin = 21, kH264SubChromaWin = 9 };   // a macroblock's windows: 16 + 5 luma rows / columns, 8 + 1 chroma

H264_HD bool h264_subpel_ok(int subpel) { return subpel == 1 || subpel == 2 || subpel == 4; }
// A vector (quarter samples) the rule admits for macroblock (mx, my): on the grid, inside the range, the whole samples around the displaced
// block (floor and ceiling of the position) inside the padded picture.  The filter taps beyond them are read clamped.
H264_HD bool h264_sub_valid(int vx, int vy, int search, int subpel, int mx, int my, int mbw, int mbh) {
    const int off = 4 / subpel - 1;
    if ((vx & off) || (vy & off) || vx < -4 * search || vx > 4 * search || vy < -4 * search || vy > 4 * search) return false;
    const int x0 = 16 * mx + (vx >> 2), x1 = 16 * mx + ((vx + 3) >> 2), y0 = 16 * my + (vy >> 2), y1 = 16 * my + ((vy + 3) >> 2);
    return x0 >= 0 && x1 + 16 <= 16 * mbw && y0 >= 0 && y1 + 16 <= 16 * mbh;
}
// The vector that is coded (the given one when it is valid, else (0, 0)), split into whole-sample offsets and fractions for both planes.
struct h264_sub_ref {
    int vx, vy;                                         // quarter luma samples = eighth chroma samples
    int ix, iy, xf, yf;                                 // luma: floor(v / 4), v & 3
    int cix, ciy, cxf, cyf;                             // chroma: floor(v / 8), v & 7
};
H264_HD h264_sub_ref h264_sub_fetch(int vx, int vy, int search, int subpel, int mx, int my, int mbw, int mbh) {
    h264_sub_ref r;
    const bool ok = h264_sub_valid(vx, vy, search, subpel, mx, my, mbw, mbh);
    r.vx = ok ? vx : 0, r.vy = ok ? vy : 0;
    r.ix = r.vx >> 2, r.iy = r.vy >> 2, r.xf = r.vx & 3, r.yf = r.vy & 3;
    r.cix = r.vx >> 3, r.ciy = r.vy >> 3, r.cxf = r.vx & 7, r.cyf = r.vy & 7;
    return r;
}
H264_HD int h264_sub_clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
// Sample i of a macroblock's clamped window: luma window sample (row i / 21, column i % 21) of the 21 x 21 samples that start two before
// the displaced block's integer position, chroma (i / 9, i % 9) of the 9 x 9 that start at it.  Offsets into the reference picture's plane.
H264_HD long long h264_sub_luma_at(const h264_sub_ref& at, int i, int mx, int my, int mbw, int mbh) {
    const int py = h264_sub_clampi(16 * my + at.iy - 2 + i / kH264SubLumaWin, 16 * mbh - 1);
    const int px = h264_sub_clampi(16 * mx + at.ix - 2 + i % kH264SubLumaWin, 16 * mbw - 1);
    return (long long)py * (16LL * mbw) + px;
}
H264_HD long long h264_sub_chroma_at(const h264_sub_ref& at, int i, int mx, int my, int mbw, int mbh) {
    const int py = h264_sub_clampi(8 * my + at.ciy + i / kH264SubChromaWin, 8 * mbh - 1);
    const int px = h264_sub_clampi(8 * mx + at.cix + i % kH264SubChromaWin, 8 * mbw - 1);
    return (long long)py * (8LL * mbw) + px;
}
// Prediction sample (x, y) of the macroblock from its staged windows (wy: 21 x 21, wc: 9 x 9 of one component)
H264_HD int h264_sub_pred_luma(const uint8_t* wy, const h264_sub_ref& at, int x, int y) {
    return h264_sub_luma(wy + (y + 2) * kH264SubLumaWin + x + 2, kH264SubLumaWin, at.xf, at.yf);
}
H264_HD int h264_sub_pred_chroma(const uint8_t* wc, const h264_sub_ref& at, int x, int y) {
    return h264_sub_chroma(wc + y * kH264SubChromaWin + x, kH264SubChromaWin, at.cxf, at.cyf);
}

// cost(v) = SAD(v) + lambda * (B(vx) + B(vy)), B(c) the length of se(c), c in quarter samples (for whole samples h264_me_cost's se(4 c))
H264_HD int h264_sub_cost(int sad, int lambda, int vx, int vy) { return sad + lambda * (h264_se_bits(vx) + h264_se_bits(vy)); }
// The total order (cost, |vx| + |vy|, vy, vx) in quarter samples as one 64-bit word: |v| <= 64, so 8 bits hold a biased component.
H264_HD unsigned long long h264_sub_key(int cost, int vx, int vy) {
    const int a = (vx < 0 ? -vx : vx) + (vy < 0 ? -vy : vy);
    return ((unsigned long long)(unsigned)cost << 32) | ((unsigned long long)a << 16) | ((unsigned long long)(vy + 64) << 8) | (unsigned long long)(vx + 64);
}
H264_HD void h264_sub_unkey(unsigned long long key, int* cost, int* vx, int* vy) {
    *cost = (int)(key >> 32), *vy = (int)((key >> 8) & 255u) - 64, *vx = (int)(key & 255u) - 64;
}

// serial: h264_gop_serial_mv with the vector (vx, vy) and the chain ``mvc`` in QUARTER samples (already through h264_sub_fetch; mb->fy /
// fc hold the interpolated prediction), so mvd = v - mvp without a scale.  Everything else is that function, statement for statement.
H264_HD void h264_gop_serial_sub(h264_gop_mb* mb, unsigned nz, bool any_cdc, bool inter, bool p_slice, h264_chain& ch, h264_mv_chain& mvc, int vx, int vy,
                                 h264_writer& w, int* skip_run) {
    int cbp_luma = 0;
    if (inter) {
        for (int i = 0; i < 4; ++i)
            if (nz & (0xfu << (4 * i))) cbp_luma |= 1 << i;
    } else if (nz & 0xffffu) {
        cbp_luma = 15;
    }
    const int cbp_chroma = (nz & 0xff0000u) ? 2 : any_cdc ? 1 : 0;
    const int mvdx = vx - mvc.vx, mvdy = vy - mvc.vy;
    if (inter && !cbp_luma && !cbp_chroma && !vx && !vy) {  // P_Skip: inferred vector (0, 0), no residual
        ++*skip_run;
        mb->mode = kH264ModeSkip;
        for (int i = 0; i < 4; ++i) ch.tcy[i] = 0;
        ch.tcc[0][0] = ch.tcc[0][1] = ch.tcc[1][0] = ch.tcc[1][1] = 0;
        mvc.vx = mvc.vy = 0;
        return;
    }
    if (p_slice) {
        h264_put_ue(w, (unsigned)*skip_run);            // mb_skip_run
        *skip_run = 0;
    }
    uint8_t tcy[16], tcc[8];
    h264_counter cnt;
    cnt.bits = 0, cnt.failed = false;
    h264_gop_code_mb_mv(mb->lev, inter, p_slice, cbp_luma, cbp_chroma, ch, mvdx, mvdy, cnt, tcy, tcc);
    if (cnt.failed || cnt.bits > 3200) {                // Annex A.3.1 / level_prefix <= 15: I_PCM
        h264_put_ue(w, p_slice ? 30u : 25u);
        while (w.n) w.put(0u, 1);                       // pcm_alignment_zero_bit
        for (int i = 0; i < 256; ++i) w.put(mb->sy[i], 8);
        for (int i = 0; i < 128; ++i) w.put(mb->sc[i], 8);
        for (int i = 0; i < 4; ++i) ch.tcy[i] = 16;
        ch.tcc[0][0] = ch.tcc[0][1] = ch.tcc[1][0] = ch.tcc[1][1] = 16;
        mb->mode = kH264ModePcm;
        mvc.vx = mvc.vy = 0;
        return;
    }
    h264_gop_code_mb_mv(mb->lev, inter, p_slice, cbp_luma, cbp_chroma, ch, mvdx, mvdy, w, tcy, tcc);
    for (int i = 0; i < 4; ++i) ch.tcy[i] = tcy[i * 4 + 3];
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 2; ++i) ch.tcc[c][i] = tcc[c * 4 + i * 2 + 1];
    mb->mode = inter ? kH264ModeInter : kH264ModeIntra;
    mvc.vx = inter ? vx : 0, mvc.vy = inter ? vy : 0;
}

// h264_gop_encode_mb_mv for a quarter-sample vector: mb->sy / sc are loaded, and in a P picture the windows wy (21 x 21) and wc (2 x 9 x 9)
// through h264_sub_luma_at / h264_sub_chroma_at; leaves mb->ry / rc.  (Host; the kernel spreads the per-sample pieces over its lanes.)
inline void h264_gop_encode_mb_sub(h264_gop_mb* mb, h264_chain& ch, h264_mv_chain& mvc, bool p_slice, int qp, const h264_sub_ref& at, const uint8_t* wy,
                                   const uint8_t* wc, h264_writer& w, int* skip_run) {
    if (p_slice) {
        for (int i = 0; i < 256; ++i) mb->fy[i] = (uint8_t)h264_sub_pred_luma(wy, at, i & 15, i >> 4);
        for (int i = 0; i < 128; ++i)
            mb->fc[i] = (uint8_t)h264_sub_pred_chroma(wc + (i >> 6) * kH264SubChromaWin * kH264SubChromaWin, at, i & 7, (i >> 3) & 7);
    }
    h264_gop_pred(mb, ch);
    bool inter = false;
    if (p_slice) {
        int si = 0, sp = 0;
        for (int b = 0; b < 16; ++b) {
            int a, c;
            h264_gop_block_sad(mb, b, &a, &c);
            si += a, sp += c;
        }
        inter = !(si < sp);
    }
    unsigned nz = 0;
    for (int b = 0; b < 24; ++b)
        if (h264_gop_block_forward(mb, b, inter, qp)) nz |= 1u << b;
    const bool any_cdc = h264_gop_dc(mb, inter, qp);
    h264_gop_serial_sub(mb, nz, any_cdc, inter, p_slice, ch, mvc, at.vx, at.vy, w, skip_run);
    for (int b = 0; b < 24; ++b) h264_gop_block_recon(mb, b, qp);
    h264_gop_chain(mb, ch);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Intra4x4 prediction for IDR pictures (sdv_hip_h264_i4.h "H.264 Intra4x4"): per macroblock I_NxN with nine modes per 4x4 block against
// today's Intra16x16 DC, I_PCM by today's two triggers.  The sixteen blocks of a macroblock are a serial chain (each predicts from the
// reconstruction of the ones before it), so the pieces below are per block: the neighbour samples of a block gathered into one edge
// array, ONE predictor that kernel, host and nothing else read them through, the winner's transform / quantisation / reconstruction,
// and the serial coder.  The kernel spreads a block's (mode, row) candidates over its lanes; h264_i4_encode_mb runs everything in
// order on the host.  Chroma, the Intra16x16 candidate and the I_PCM writing are the GOP path's functions.  Nothing above is touched.
// ------------------------------------------------------------------------------------------------------------------------------------
enum { kH264ModeI4 = 4 };                               // h264_gop_mb::mode of an I_NxN macroblock (its chroma is that of kH264ModeIntra)
enum { kH264I4Top = 1, kH264I4Left = 2, kH264I4Corner = 4, kH264I4TopRight = 8 };
enum { kH264I4Modes = 9, kH264I4Dc = 2 };

// coded_block_pattern -> codeNum of me(v), intra column of Table 9-4 (ChromaArrayType 1): the inverse of
// 47 31 15 0 23 27 29 30 7 11 13 14 39 43 45 46 16 3 5 10 12 19 21 26 28 35 37 42 44 1 2 4 8 17 18 20 24 6 9 22 25 32 33 34 36 40 38 41
H264_HD int h264_cbp_intra_code(int cbp) {
    const uint8_t t[48] = {3,  29, 30, 17, 31, 18, 37, 8,  32, 38, 19, 9,  20, 10, 11, 2,  16, 33, 34, 21, 35, 22, 39, 4,
                           36, 40, 23, 5,  24, 6,  7,  1,  41, 42, 43, 25, 44, 26, 46, 12, 45, 47, 27, 13, 28, 14, 15, 0};
    return t[cbp];
}

// What a macroblock of an IDR picture hands to its right neighbour: the GOP path's chain plus the Intra4x4PredMode of its four right-hand
// blocks (2 when it was coded Intra16x16 or I_PCM).
struct h264_i4_chain {
    h264_chain ch;
    uint8_t mode[4];
};

// The Intra4x4 state of one macroblock that the pieces share (LDS in the kernel), beside its h264_gop_mb.
struct h264_i4_mb {
    uint8_t edge[16];                                   // the current block's neighbours: [0] p[-1,-1], [1 + x] p[x,-1] (x 0..7), [9 + y] p[-1,y]
    uint8_t lcol[16], lmode[4];                         // the left neighbour's right column and right-hand modes (the chain)
    uint8_t mode[16];                                   // the winners so far, [by * 4 + bx]
    uint8_t pmode[16];                                  // the predicted mode of every block, [luma4x4BlkIdx]
    int avail;                                          // kH264I4* of the current block
    int have;                                           // a left neighbour exists
    int cost;                                           // sum of the winners' costs
    unsigned nz;                                        // bit b: block b (luma4x4BlkIdx) has a nonzero level
};

// Which neighbours 4x4 block (bx, by) has: the row above the macroblock is another slice, so "top" needs by >= 1.
H264_HD int h264_i4_avail(int bx, int by, bool have_left) {
    const bool top = by >= 1, left = bx >= 1 || have_left;
    const bool tr = top && bx <= 2 && !(bx == 1 && (by == 1 || by == 3));
    return (top ? kH264I4Top : 0) | (left ? kH264I4Left : 0) | (top && left ? kH264I4Corner : 0) | (tr ? kH264I4TopRight : 0);
}
// V, DDL, VL need top; H, HU left; DDR, VR, HD top, left and corner; DC nothing.
H264_HD bool h264_i4_mode_ok(int mode, int avail) {
    const uint8_t need[kH264I4Modes] = {1, 2, 0, 1, 7, 7, 7, 1, 2};
    return (avail & need[mode]) == need[mode];
}

// serial: the neighbours of block b from the macroblock's reconstruction so far and the chain's left column, never from HBM.  Top-right
// samples that are not available repeat p[3,-1] (8.3.1.2); samples of a missing side are 128 and read by no admitted mode but DC's sums,
// which skip them.
H264_HD void h264_i4_edges(const uint8_t* ry, h264_i4_mb* s, int b) {
    int x0, y0;
    h264_gop_block_xy(b, &x0, &y0);
    const int avail = h264_i4_avail(x0 >> 2, y0 >> 2, s->have != 0);
    s->avail = avail;
    for (int i = 0; i < 13; ++i) s->edge[i] = 128;
    if (avail & kH264I4Top) {
        for (int i = 0; i < 4; ++i) s->edge[1 + i] = ry[(y0 - 1) * 16 + x0 + i];
        for (int i = 4; i < 8; ++i) s->edge[1 + i] = (avail & kH264I4TopRight) ? ry[(y0 - 1) * 16 + x0 + i] : s->edge[4];
    }
    if (avail & kH264I4Left)
        for (int i = 0; i < 4; ++i) s->edge[9 + i] = x0 ? ry[(y0 + i) * 16 + x0 - 1] : s->lcol[y0 + i];
    if (avail & kH264I4Corner) s->edge[0] = x0 ? ry[(y0 - 1) * 16 + x0 - 1] : s->lcol[y0 - 1];
}

// THE predictor (8.3.1.2.1 - 8.3.1.2.9): sample (x, y) of the block in `mode` from an edge array.  p[i,-1] = t(i), i = -1 .. 7;
// p[-1,j] = l(j), j = -1 .. 3; both reach the corner at -1.
H264_HD int h264_i4_t(const uint8_t* e, int i) { return e[1 + i]; }
H264_HD int h264_i4_l(const uint8_t* e, int j) { return j < 0 ? e[0] : e[9 + j]; }
H264_HD int h264_i4_f3(int a, int b, int c) { return (a + 2 * b + c + 2) >> 2; }
H264_HD int h264_i4_pred(const uint8_t* e, int avail, int mode, int x, int y) {
    switch (mode) {
    case 0: return h264_i4_t(e, x);
    case 1: return h264_i4_l(e, y);
    case 2: {
        const int st = e[1] + e[2] + e[3] + e[4], sl = e[9] + e[10] + e[11] + e[12];
        const bool top = (avail & kH264I4Top) != 0, left = (avail & kH264I4Left) != 0;
        return top && left ? (st + sl + 4) >> 3 : top ? (st + 2) >> 2 : left ? (sl + 2) >> 2 : 128;
    }
    case 3:
        if (x == 3 && y == 3) return (h264_i4_t(e, 6) + 3 * h264_i4_t(e, 7) + 2) >> 2;
        return h264_i4_f3(h264_i4_t(e, x + y), h264_i4_t(e, x + y + 1), h264_i4_t(e, x + y + 2));
    case 4:
        if (x > y) return h264_i4_f3(h264_i4_t(e, x - y - 2), h264_i4_t(e, x - y - 1), h264_i4_t(e, x - y));
        if (x < y) return h264_i4_f3(h264_i4_l(e, y - x - 2), h264_i4_l(e, y - x - 1), h264_i4_l(e, y - x));
        return h264_i4_f3(h264_i4_t(e, 0), e[0], h264_i4_l(e, 0));
    case 5: {
        const int z = 2 * x - y, i = x - (y >> 1);
        if (z >= 0 && !(z & 1)) return (h264_i4_t(e, i - 1) + h264_i4_t(e, i) + 1) >> 1;
        if (z > 0) return h264_i4_f3(h264_i4_t(e, i - 2), h264_i4_t(e, i - 1), h264_i4_t(e, i));
        if (z == -1) return h264_i4_f3(h264_i4_l(e, 0), e[0], h264_i4_t(e, 0));
        return h264_i4_f3(h264_i4_l(e, y - 1), h264_i4_l(e, y - 2), h264_i4_l(e, y - 3));
    }
    case 6: {
        const int z = 2 * y - x, j = y - (x >> 1);
        if (z >= 0 && !(z & 1)) return (h264_i4_l(e, j - 1) + h264_i4_l(e, j) + 1) >> 1;
        if (z > 0) return h264_i4_f3(h264_i4_l(e, j - 2), h264_i4_l(e, j - 1), h264_i4_l(e, j));
        if (z == -1) return h264_i4_f3(h264_i4_l(e, 0), e[0], h264_i4_t(e, 0));
        return h264_i4_f3(h264_i4_t(e, x - 1), h264_i4_t(e, x - 2), h264_i4_t(e, x - 3));
    }
    case 7: {
        const int i = x + (y >> 1);
        if (!(y & 1)) return (h264_i4_t(e, i) + h264_i4_t(e, i + 1) + 1) >> 1;
        return h264_i4_f3(h264_i4_t(e, i), h264_i4_t(e, i + 1), h264_i4_t(e, i + 2));
    }
    default: {
        const int z = x + 2 * y, j = y + (x >> 1);
        if (z > 5) return h264_i4_l(e, 3);
        if (z == 5) return (h264_i4_l(e, 2) + 3 * h264_i4_l(e, 3) + 2) >> 2;
        if (!(z & 1)) return (h264_i4_l(e, j) + h264_i4_l(e, j + 1) + 1) >> 1;
        return h264_i4_f3(h264_i4_l(e, j), h264_i4_l(e, j + 1), h264_i4_l(e, j + 2));
    }
    }
}

// predIntra4x4PredMode of block (bx, by) (8.3.1.1): min(left, top), 2 when either is missing; an Intra16x16 / I_PCM neighbour counts as 2
// (the chain says so).  The block above the macroblock's top row is another slice, so the top row always predicts 2.
H264_HD int h264_i4_pred_mode(const h264_i4_mb* s, int bx, int by) {
    const int a = bx ? s->mode[by * 4 + bx - 1] : s->have ? s->lmode[by] : -1;
    const int t = by ? s->mode[(by - 1) * 4 + bx] : -1;
    return (a < 0 || t < 0) ? kH264I4Dc : a < t ? a : t;
}
// cost = SAD + lambda * (1 if the mode is the predicted one else 4), and the order (cost, mode) as one word (cost < 2^13)
H264_HD unsigned h264_i4_key(int sad, int lambda, int mode, int pmode) { return ((unsigned)(sad + lambda * (mode == pmode ? 1 : 4)) << 4) | (unsigned)mode; }

// serial: the state at the start of a macroblock - the Intra16x16 / chroma DC predictors, the chain's column and modes, block 0's edges
H264_HD void h264_i4_begin(h264_gop_mb* mb, h264_i4_mb* s, const h264_i4_chain& ch) {
    h264_gop_pred(mb, ch.ch);
    s->have = ch.ch.have;
    for (int i = 0; i < 16; ++i) s->lcol[i] = ch.ch.have ? ch.ch.ycol[i] : 128;
    for (int i = 0; i < 4; ++i) s->lmode[i] = ch.ch.have ? ch.mode[i] : kH264I4Dc;
    for (int i = 0; i < 16; ++i) s->mode[i] = s->pmode[i] = kH264I4Dc;
    s->cost = 0, s->nz = 0;
    h264_i4_edges(mb->ry, s, 0);
}
// The Intra16x16 candidate's cost: sum |src - DC16|, DC16 the macroblock's own DC - the rounded mean of its 256 source samples.  (What the
// left neighbour's column mispredicts of that mean goes into the one Intra16x16 DC level, not into sixteen blocks; measured against the
// predictor instead, a flat macroblock without a left neighbour would pay its offset from 128 sixteen times and turn I_NxN.)
// per luma block: its part of the sum of the samples, and of the SAD against dc16 = h264_i4_dc16(sum of the sums)
H264_HD int h264_i4_block_sum(const h264_gop_mb* mb, int b) {
    int x, y, sum = 0;
    h264_gop_block_xy(b, &x, &y);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) sum += mb->sy[(y + i) * 16 + x + j];
    return sum;
}
H264_HD int h264_i4_dc16(int sum) { return (sum + 128) >> 8; }
H264_HD int h264_i4_block_sad16(const h264_gop_mb* mb, int b, int dc16) {
    int x, y, sum = 0;
    h264_gop_block_xy(b, &x, &y);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const int d = (int)mb->sy[(y + i) * 16 + x + j] - dc16;
            sum += d < 0 ? -d : d;
        }
    return sum;
}
// one row of one candidate: SAD of the 4 samples of row `row` of block b against mode `mode` (the kernel's lanes own one each)
H264_HD int h264_i4_row_sad(const h264_gop_mb* mb, const h264_i4_mb* s, int b, int mode, int row) {
    int x, y, sum = 0;
    h264_gop_block_xy(b, &x, &y);
    for (int j = 0; j < 4; ++j) {
        const int d = (int)mb->sy[(y + row) * 16 + x + j] - h264_i4_pred(s->edge, s->avail, mode, j, row);
        sum += d < 0 ? -d : d;
    }
    return sum;
}
// serial: the winner of block b (key = h264_i4_key of the minimum) - prediction, residual, transform, quantisation with the intra dead
// zone, all 16 levels to lev block 1 + b (scan order), dequantisation, reconstruction into mb->ry; then the edges of block b + 1.
H264_HD void h264_i4_block_code(h264_gop_mb* mb, h264_i4_mb* s, int b, unsigned key, int qp) {
    int x0, y0, pr[16], xs[16], w[16], d[16], r[16];
    h264_gop_block_xy(b, &x0, &y0);
    const int mode = (int)(key & 15u);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            pr[i * 4 + j] = h264_i4_pred(s->edge, s->avail, mode, j, i);
            xs[i * 4 + j] = (int)mb->sy[(y0 + i) * 16 + x0 + j] - pr[i * 4 + j];
        }
    h264_forward4x4(xs, w);
    const int q6 = qp % 6, k = qp / 6, qbits = 15 + k, f = (1 << qbits) / 3;
    int16_t* lv = mb->lev + (1 + b) * 16;
    bool any = false;
    for (int ras = 0; ras < 16; ++ras) {
        const int cls = h264_pos_class(ras >> 2, ras & 3);
        const int l = h264_quant(w[ras], h264_mf(q6, cls), f, qbits);
        lv[h264_scan_pos(ras)] = (int16_t)l;
        d[ras] = l * h264_norm(q6, cls) * (1 << k);
        if (l) any = true;
    }
    mb->dcw[b] = w[0];
    h264_inverse4x4(d, r);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) mb->ry[(y0 + i) * 16 + x0 + j] = (uint8_t)h264_clip255(pr[i * 4 + j] + r[i * 4 + j]);
    s->pmode[b] = (uint8_t)h264_i4_pred_mode(s, x0 >> 2, y0 >> 2);
    s->mode[(y0 >> 2) * 4 + (x0 >> 2)] = (uint8_t)mode;
    s->cost += (int)(key >> 4);
    if (any) s->nz |= 1u << b;
    if (b < 15) h264_i4_edges(mb->ry, s, b + 1);
}

// macroblock_layer() of an I_NxN macroblock: mb_type, the sixteen mode symbols, chroma mode, cbp by the intra column, the residual
template <class Sink>
H264_HD void h264_i4_code_mb(const int16_t* lev, const h264_i4_mb* s, int cbp_luma, int cbp_chroma, const h264_chain& left, Sink& sk, uint8_t* tcy,
                             uint8_t* tcc) {
    for (int i = 0; i < 16; ++i) tcy[i] = 0;            // [by * 4 + bx]
    for (int i = 0; i < 8; ++i) tcc[i] = 0;             // [c * 4 + by * 2 + bx]
    h264_put_ue(sk, 0u);                                // mb_type I_NxN (no transform_size_8x8_flag: the PPS has no 8x8 transform)
    for (int b = 0; b < 16; ++b) {
        const int bx = 2 * ((b >> 2) & 1) + (b & 1), by = 2 * (b >> 3) + ((b >> 1) & 1);
        const int mode = s->mode[by * 4 + bx], pm = s->pmode[b];
        if (mode == pm) sk.put(1u, 1);                  // prev_intra4x4_pred_mode_flag
        else sk.put(0u, 1), sk.put((unsigned)(mode < pm ? mode : mode - 1), 3);     // rem_intra4x4_pred_mode
    }
    h264_put_ue(sk, 0u);                                // intra_chroma_pred_mode: DC
    h264_put_ue(sk, (unsigned)h264_cbp_intra_code(cbp_luma + 16 * cbp_chroma));
    if (cbp_luma || cbp_chroma) h264_put_se(sk, 0);     // mb_qp_delta
    for (int b = 0; b < 16; ++b) {
        if (!((cbp_luma >> (b >> 2)) & 1)) continue;
        const int bx = 2 * ((b >> 2) & 1) + (b & 1), by = 2 * (b >> 3) + ((b >> 1) & 1);
        const int a = bx ? tcy[by * 4 + bx - 1] : left.have ? left.tcy[by] : -1;
        const int t = by ? tcy[(by - 1) * 4 + bx] : -1;
        tcy[by * 4 + bx] = (uint8_t)h264_code_block(lev + (1 + b) * 16, 16, h264_nc(a, t), sk);
    }
    h264_gop_code_chroma(lev, cbp_chroma, left, sk, tcc);
}

// serial: after the sixteen blocks and the chroma levels - the decision I_NxN against Intra16x16 (use_i4: sum of costs < SAD against the
// macroblock's DC; otherwise the caller left the Intra16x16 levels in place), the counting pass, the I_PCM decision, the bits; leaves mb->mode and the
// chain's TotalCoeffs and modes.  nz: the ballot of h264_gop_block_forward (luma bits only when !use_i4).
H264_HD void h264_i4_serial(h264_gop_mb* mb, const h264_i4_mb* s, bool use_i4, unsigned nz, bool any_cdc, h264_i4_chain& ch, h264_writer& w) {
    for (int i = 0; i < 4; ++i) ch.mode[i] = kH264I4Dc;
    if (!use_i4) {
        int skip_run = 0;
        h264_gop_serial(mb, nz, any_cdc, false, false, ch.ch, w, &skip_run);
        return;
    }
    int cbp_luma = 0;
    for (int i = 0; i < 4; ++i)
        if (s->nz & (0xfu << (4 * i))) cbp_luma |= 1 << i;
    const int cbp_chroma = (nz & 0xff0000u) ? 2 : any_cdc ? 1 : 0;
    uint8_t tcy[16], tcc[8];
    h264_counter cnt;
    cnt.bits = 0, cnt.failed = false;
    h264_i4_code_mb(mb->lev, s, cbp_luma, cbp_chroma, ch.ch, cnt, tcy, tcc);
    if (cnt.failed || cnt.bits > 3200) {                // Annex A.3.1 / level_prefix <= 15: I_PCM
        h264_put_ue(w, 25u);
        while (w.n) w.put(0u, 1);                       // pcm_alignment_zero_bit
        for (int i = 0; i < 256; ++i) w.put(mb->sy[i], 8);
        for (int i = 0; i < 128; ++i) w.put(mb->sc[i], 8);
        for (int i = 0; i < 4; ++i) ch.ch.tcy[i] = 16;
        ch.ch.tcc[0][0] = ch.ch.tcc[0][1] = ch.ch.tcc[1][0] = ch.ch.tcc[1][1] = 16;
        mb->mode = kH264ModePcm;
        return;
    }
    h264_i4_code_mb(mb->lev, s, cbp_luma, cbp_chroma, ch.ch, w, tcy, tcc);
    for (int i = 0; i < 4; ++i) ch.ch.tcy[i] = tcy[i * 4 + 3];
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 2; ++i) ch.ch.tcc[c][i] = tcc[c * 4 + i * 2 + 1];
    for (int i = 0; i < 4; ++i) ch.mode[i] = s->mode[i * 4 + 3];
    mb->mode = kH264ModeI4;
}
// per block: reconstruction after the serial part - an I_NxN macroblock's luma already stands in mb->ry
H264_HD void h264_i4_block_recon(h264_gop_mb* mb, int b, int qp) {
    if (mb->mode == kH264ModeI4 && b < 16) return;
    h264_gop_block_recon(mb, b, qp);
}

// The whole macroblock step of an IDR picture in order (host; the kernel spreads the candidates and the per-block pieces over its lanes).
// mb->sy / sc are loaded; leaves mb->ry / rc.  Returns mb->mode.
inline int h264_i4_encode_mb(h264_gop_mb* mb, h264_i4_mb* s, h264_i4_chain& ch, int qp, h264_writer& w) {
    h264_i4_begin(mb, s, ch);
    const int lambda = h264_me_lambda(qp);
    int sum = 0, sad16 = 0;
    for (int b = 0; b < 16; ++b) sum += h264_i4_block_sum(mb, b);
    for (int b = 0; b < 16; ++b) sad16 += h264_i4_block_sad16(mb, b, h264_i4_dc16(sum));
    for (int b = 0; b < 16; ++b) {
        int x, y;
        h264_gop_block_xy(b, &x, &y);
        const int pm = h264_i4_pred_mode(s, x >> 2, y >> 2);
        unsigned best = 0xffffffffu;
        for (int mode = 0; mode < kH264I4Modes; ++mode) {
            if (!h264_i4_mode_ok(mode, s->avail)) continue;
            int sad = 0;
            for (int row = 0; row < 4; ++row) sad += h264_i4_row_sad(mb, s, b, mode, row);
            const unsigned key = h264_i4_key(sad, lambda, mode, pm);
            if (key < best) best = key;
        }
        h264_i4_block_code(mb, s, b, best, qp);
    }
    const bool use_i4 = s->cost < sad16;
    unsigned nz = 0;
    for (int b = use_i4 ? 16 : 0; b < 24; ++b)
        if (h264_gop_block_forward(mb, b, false, qp)) nz |= 1u << b;
    const bool any_cdc = h264_gop_dc(mb, false, qp);
    h264_i4_serial(mb, s, use_i4, nz, any_cdc, ch, w);
    for (int b = 0; b < 24; ++b) h264_i4_block_recon(mb, b, qp);
    h264_gop_chain(mb, ch.ch);
    return mb->mode;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// In-loop deblocking filter (sdv_hip_h264_lf.h "H.264 deblocking"): 8.7 for frame macroblocks, 4:2:0, no 8x8 transform, filterOffsetA =
// filterOffsetB = 0, one reference picture.  The pieces below are per line of one edge: the side information word of a macroblock, bS,
// the index into the tables, and the one sample filter.  The kernel gives a line to a lane (an LDS window of the macroblock and its
// neighbours); h264_lf_picture walks the macroblocks in raster order on the planes themselves.  Above, only the two slice header
// functions changed: a defaulted argument ``deblock`` that switches the filter on in the header.
// ------------------------------------------------------------------------------------------------------------------------------------
// mbinfo word of a macroblock: bits 0 .. 15 bit 4 by + bx set when luma block (bx, by) of an INTER macroblock kept a nonzero level (0 in
// every other macroblock); bit 16 intra (Intra16x16, I_NxN, I_PCM); bit 17 I_PCM; bit 18 the coded vector is (0, 0) whatever ``mv``
// holds (P_Skip, or a vector the stream rule did not admit); bits 19 .. 31 zero.
enum { kH264LfIntra = 1 << 16, kH264LfPcm = 1 << 17, kH264LfZeroMv = 1 << 18 };

H264_HD unsigned h264_lf_nz_raster(unsigned nz) {       // bit luma4x4BlkIdx -> bit 4 by + bx
    unsigned r = 0;
    for (int b = 0; b < 16; ++b) {
        int x, y;
        h264_gop_block_xy(b, &x, &y);
        if ((nz >> b) & 1u) r |= 1u << (y + (x >> 2));
    }
    return r;
}
// mode: h264_gop_mb::mode after the serial piece; nz: the ballot of h264_gop_block_forward; (vx, vy): the vector that was coded
H264_HD uint32_t h264_lf_word(int mode, unsigned nz, int vx, int vy) {
    if (mode == kH264ModePcm) return (uint32_t)(kH264LfIntra | kH264LfPcm);
    if (mode == kH264ModeIntra || mode == kH264ModeI4) return (uint32_t)kH264LfIntra;
    return (mode == kH264ModeInter ? h264_lf_nz_raster(nz & 0xffffu) : 0u) | (!vx && !vy ? (uint32_t)kH264LfZeroMv : 0u);
}

H264_HD int h264_lf_alpha(int index) {                  // Table 8-16, alpha'
    const uint8_t t[52] = {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  4,  4,  5,  6,  7,  8,   9,   10,  12,  13,
                           15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144, 162, 182, 203, 226, 255, 255};
    return t[index];
}
H264_HD int h264_lf_beta(int index) {                   // Table 8-16, beta'
    const uint8_t t[52] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,  0,  0,  0,  0,  0,  2,  2,  2,  3,  3,  3,  3,  4,  4,  4,
                           6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18};
    return t[index];
}
H264_HD int h264_lf_tc0(int index, int bS) {            // Table 8-17, tC0' for bS 1, 2, 3
    const uint8_t t[3][52] = {
        {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6, 6, 7, 8, 9, 10, 11, 13},
        {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 5, 5, 6, 7, 8, 8, 10, 11, 12, 13, 15, 17},
        {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 23, 25}};
    return t[bS - 1][index];
}

// One side of an edge: the macroblock's word and its vector in QUARTER samples ((0, 0) for an intra macroblock and under bit 18).
// ``mv`` holds even whole samples without subpel and quarter samples with it.
struct h264_lf_side {
    uint32_t info;
    int vx, vy;
};
H264_HD h264_lf_side h264_lf_side_of(uint32_t info, const int16_t* v, int subpel) {
    h264_lf_side s;
    const bool zero = (info & (uint32_t)(kH264LfIntra | kH264LfZeroMv)) != 0;
    const int scale = subpel ? 1 : 4;
    s.info = info;
    s.vx = zero ? 0 : (int)v[0] * scale, s.vy = zero ? 0 : (int)v[1] * scale;
    return s;
}
// bS of the edge between luma block pblk of P and qblk of Q (4 by + bx each); mb_edge: the two lie in different macroblocks
H264_HD int h264_lf_bs(const h264_lf_side& p, int pblk, const h264_lf_side& q, int qblk, bool mb_edge) {
    if ((p.info | q.info) & (uint32_t)kH264LfIntra) return mb_edge ? 4 : 3;
    if (((p.info >> pblk) | (q.info >> qblk)) & 1u) return 2;
    const int dx = p.vx - q.vx, dy = p.vy - q.vy;
    return (dx >= 4 || dx <= -4 || dy >= 4 || dy <= -4) ? 1 : 0;
}
// indexA = indexB of an edge: qPp / qPq are 0 for I_PCM and the slice qp otherwise, each through Table 8-15 first for chroma
H264_HD int h264_lf_index(const h264_lf_side& p, const h264_lf_side& q, int qp, bool chroma) {
    int a = (p.info & (uint32_t)kH264LfPcm) ? 0 : qp, b = (q.info & (uint32_t)kH264LfPcm) ? 0 : qp;
    if (chroma) a = h264_qpc(a), b = h264_qpc(b);
    const int i = (a + b + 1) >> 1;
    return i < 0 ? 0 : i > 51 ? 51 : i;
}
// 8.7.2.3 / 8.7.2.4 for one line: q0 at ``q``, q_i at q[i * step], p_i at q[-(i + 1) * step].  bS 1 .. 4.
H264_HD void h264_lf_line(uint8_t* q, int step, int bS, int index, bool chroma) {
    const int alpha = h264_lf_alpha(index), beta = h264_lf_beta(index);
    const int p0 = q[-step], p1 = q[-2 * step], q0 = q[0], q1 = q[step];
    const int d0 = p0 - q0, dp = p1 - p0, dq = q1 - q0;
    if (!((d0 < 0 ? -d0 : d0) < alpha && (dp < 0 ? -dp : dp) < beta && (dq < 0 ? -dq : dq) < beta)) return;
    if (chroma) {
        if (bS < 4) {
            const int tc = h264_lf_tc0(index, bS) + 1;
            int delta = (((q0 - p0) * 4) + (p1 - q1) + 4) >> 3;
            delta = delta < -tc ? -tc : delta > tc ? tc : delta;
            q[-step] = (uint8_t)h264_clip255(p0 + delta), q[0] = (uint8_t)h264_clip255(q0 - delta);
        } else {
            q[-step] = (uint8_t)((2 * p1 + p0 + q1 + 2) >> 2), q[0] = (uint8_t)((2 * q1 + q0 + p1 + 2) >> 2);
        }
        return;
    }
    const int p2 = q[-3 * step], q2 = q[2 * step];
    const int ap = p2 - p0 < 0 ? p0 - p2 : p2 - p0, aq = q2 - q0 < 0 ? q0 - q2 : q2 - q0;
    if (bS < 4) {
        const int tc0 = h264_lf_tc0(index, bS), tc = tc0 + (ap < beta ? 1 : 0) + (aq < beta ? 1 : 0);
        int delta = (((q0 - p0) * 4) + (p1 - q1) + 4) >> 3;
        delta = delta < -tc ? -tc : delta > tc ? tc : delta;
        q[-step] = (uint8_t)h264_clip255(p0 + delta), q[0] = (uint8_t)h264_clip255(q0 - delta);
        if (ap < beta) {
            int d = (p2 + ((p0 + q0 + 1) >> 1) - 2 * p1) >> 1;
            d = d < -tc0 ? -tc0 : d > tc0 ? tc0 : d;
            q[-2 * step] = (uint8_t)(p1 + d);
        }
        if (aq < beta) {
            int d = (q2 + ((p0 + q0 + 1) >> 1) - 2 * q1) >> 1;
            d = d < -tc0 ? -tc0 : d > tc0 ? tc0 : d;
            q[step] = (uint8_t)(q1 + d);
        }
        return;
    }
    const bool small = (d0 < 0 ? -d0 : d0) < (alpha >> 2) + 2;
    if (ap < beta && small) {
        const int p3 = q[-4 * step];
        q[-step] = (uint8_t)((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3);
        q[-2 * step] = (uint8_t)((p2 + p1 + p0 + q0 + 2) >> 2);
        q[-3 * step] = (uint8_t)((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3);
    } else {
        q[-step] = (uint8_t)((2 * p1 + p0 + q1 + 2) >> 2);
    }
    if (aq < beta && small) {
        const int q3 = q[3 * step];
        q[0] = (uint8_t)((p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3);
        q[step] = (uint8_t)((p0 + q0 + q1 + q2 + 2) >> 2);
        q[2 * step] = (uint8_t)((2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3);
    } else {
        q[0] = (uint8_t)((2 * q1 + q0 + p1 + 2) >> 2);
    }
}
// Line l (0 .. 15) of luma edge e (0 .. 3) of macroblock Q, whose sample (0, 0) is mb[0] in rows of ``stride``: dir 0 the vertical edge
// at column 4 e (l a row), dir 1 the horizontal edge at row 4 e (l a column).  p: the left / upper neighbour for e = 0, Q itself else.
H264_HD void h264_lf_luma_line(uint8_t* mb, int stride, int dir, int e, int l, const h264_lf_side& p, const h264_lf_side& q, int qp) {
    const int along = l >> 2, pe = e ? e - 1 : 3;
    const int qblk = dir ? 4 * e + along : 4 * along + e, pblk = dir ? 4 * pe + along : 4 * along + pe;
    const int bS = h264_lf_bs(p, pblk, q, qblk, e == 0);
    if (!bS) return;
    h264_lf_line(dir ? mb + 4 * e * stride + l : mb + l * stride + 4 * e, dir ? stride : 1, bS, h264_lf_index(p, q, qp, false), false);
}
// Line l (0 .. 7) of chroma edge c (0, 1: chroma column / row 4 c) of one chroma plane of macroblock Q: its bS is that of luma edge 2 c at
// the luma lines 2 l and 2 l + 1, which lie in one 4x4 block.
H264_HD void h264_lf_chroma_line(uint8_t* mb, int stride, int dir, int c, int l, const h264_lf_side& p, const h264_lf_side& q, int qp) {
    const int e = 2 * c, along = l >> 1, pe = e ? e - 1 : 3;
    const int qblk = dir ? 4 * e + along : 4 * along + e, pblk = dir ? 4 * pe + along : 4 * along + pe;
    const int bS = h264_lf_bs(p, pblk, q, qblk, e == 0);
    if (!bS) return;
    h264_lf_line(dir ? mb + 4 * c * stride + l : mb + l * stride + 4 * c, dir ? stride : 1, bS, h264_lf_index(p, q, qp, true), true);
}

// The whole filter of one picture in the standard's order, on the planes themselves (host): macroblocks in raster order; in each luma
// vertical edges left to right, luma horizontal edges top to bottom, then the same for Cb and for Cr.  The left and top picture edges are
// not filtered.  info [mbh * mbw], mv [mbh * mbw * 2].
inline void h264_lf_picture(uint8_t* ry, uint8_t* rcb, uint8_t* rcr, int mbh, int mbw, int qp, const uint32_t* info, const int16_t* mv, int subpel) {
    const int lw = 16 * mbw, cw = 8 * mbw;
    for (int my = 0; my < mbh; ++my)
        for (int mx = 0; mx < mbw; ++mx) {
            const int at = my * mbw + mx;
            const h264_lf_side q = h264_lf_side_of(info[at], mv + 2 * at, subpel);
            const h264_lf_side left = mx ? h264_lf_side_of(info[at - 1], mv + 2 * (at - 1), subpel) : q;
            const h264_lf_side up = my ? h264_lf_side_of(info[at - mbw], mv + 2 * (at - mbw), subpel) : q;
            uint8_t* y0 = ry + (long long)my * 16 * lw + mx * 16;
            for (int dir = 0; dir < 2; ++dir)
                for (int e = 0; e < 4; ++e) {
                    if (e == 0 && !(dir ? my : mx)) continue;
                    for (int l = 0; l < 16; ++l) h264_lf_luma_line(y0, lw, dir, e, l, e ? q : dir ? up : left, q, qp);
                }
            for (int c = 0; c < 2; ++c) {
                uint8_t* c0 = (c ? rcr : rcb) + (long long)my * 8 * cw + mx * 8;
                for (int dir = 0; dir < 2; ++dir)
                    for (int e = 0; e < 2; ++e) {
                        if (e == 0 && !(dir ? my : mx)) continue;
                        for (int l = 0; l < 8; ++l) h264_lf_chroma_line(c0, cw, dir, e, l, e ? q : dir ? up : left, q, qp);
                    }
            }
        }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Macroblock partitions (sdv_hip_h264_part.h "H.264 partitions"): four vectors per inter macroblock, one per 8x8 luma quadrant
// (mbPartIdx 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right), always in QUARTER samples; P_8x8 with four P_L0_8x8 sub types
// where they differ, today's P_Skip / P_L0_16x16 where they are equal.  The pieces below are what the search kernel, the per-position
// kernel, the filter and the host share: the admission of a vector at every subpel (0 included), the per-partition clamped windows
// (read through the interpolators above), the vector prediction of 8.4.1.3 for 8x8 partitions in this slice layout, the macroblock
// writer, the search's decision, and bS with four vectors a side.  Nothing above is touched.
// ------------------------------------------------------------------------------------------------------------------------------------
enum { kH264PartLumaWin = 13, kH264PartChromaWin = 5 }; // a partition's windows: 8 + 5 luma rows / columns, 4 + 1 chroma
enum { kH264LfZeroPart0 = 1 << 19 };                    // bits 19 .. 22: the coded vector of partition i is (0, 0) whatever ``mv`` holds

H264_HD bool h264_part_subpel_ok(int subpel) { return subpel == 0 || h264_subpel_ok(subpel); }
// A vector (quarter samples) the rule admits for macroblock (mx, my) - the macroblock's own 16x16 rule, for every partition.  subpel 0:
// every component a multiple of 8 (the even whole-sample grid of sdv_hip_ext.h); 1, 2, 4: h264_sub_valid.
H264_HD bool h264_part_valid(int vx, int vy, int search, int subpel, int mx, int my, int mbw, int mbh) {
    if (subpel == 0) return !(vx & 7) && !(vy & 7) && h264_sub_valid(vx, vy, search, 1, mx, my, mbw, mbh);
    return h264_sub_valid(vx, vy, search, subpel, mx, my, mbw, mbh);
}
// The vector that is coded for a partition (the given one when it is valid, else (0, 0)), split as h264_sub_fetch splits it.
H264_HD h264_sub_ref h264_part_fetch(int vx, int vy, int search, int subpel, int mx, int my, int mbw, int mbh) {
    const bool ok = h264_part_valid(vx, vy, search, subpel, mx, my, mbw, mbh);
    return h264_sub_fetch(ok ? vx : 0, ok ? vy : 0, search, 4, mx, my, mbw, mbh);   // (a valid vector lies on the quarter grid too)
}
// Sample i of partition ``part``'s clamped window: luma (row i / 13, column i % 13) of the 13 x 13 samples that start two before the
// displaced 8x8 block's integer position, chroma (i / 5, i % 5) of the 5 x 5 that start at the displaced 4x4 block.  Offsets into the plane.
H264_HD long long h264_part_luma_at(const h264_sub_ref& at, int part, int i, int mx, int my, int mbw, int mbh) {
    const int py = h264_sub_clampi(16 * my + 8 * (part >> 1) + at.iy - 2 + i / kH264PartLumaWin, 16 * mbh - 1);
    const int px = h264_sub_clampi(16 * mx + 8 * (part & 1) + at.ix - 2 + i % kH264PartLumaWin, 16 * mbw - 1);
    return (long long)py * (16LL * mbw) + px;
}
H264_HD long long h264_part_chroma_at(const h264_sub_ref& at, int part, int i, int mx, int my, int mbw, int mbh) {
    const int py = h264_sub_clampi(8 * my + 4 * (part >> 1) + at.ciy + i / kH264PartChromaWin, 8 * mbh - 1);
    const int px = h264_sub_clampi(8 * mx + 4 * (part & 1) + at.cix + i % kH264PartChromaWin, 8 * mbw - 1);
    return (long long)py * (8LL * mbw) + px;
}
// Prediction sample (x, y) of the MACROBLOCK (luma 0 .. 15, chroma 0 .. 7) from the four staged windows of its partitions
// (wy: [4][13 x 13], wc: [4][5 x 5] of one component), at: the four fetched vectors
H264_HD int h264_part_pred_luma(const uint8_t* wy, const h264_sub_ref* at, int x, int y) {
    const int part = 2 * (y >> 3) + (x >> 3);
    return h264_sub_luma(wy + part * kH264PartLumaWin * kH264PartLumaWin + ((y & 7) + 2) * kH264PartLumaWin + (x & 7) + 2, kH264PartLumaWin,
                         at[part].xf, at[part].yf);
}
H264_HD int h264_part_pred_chroma(const uint8_t* wc, const h264_sub_ref* at, int x, int y) {
    const int part = 2 * (y >> 2) + (x >> 2);
    return h264_sub_chroma(wc + part * kH264PartChromaWin * kH264PartChromaWin + (y & 3) * kH264PartChromaWin + (x & 3), kH264PartChromaWin,
                           at[part].cxf, at[part].cyf);
}

// What a macroblock hands to its right neighbour for 8.4.1.3: the vectors of its partitions 1 (v[0], neighbour A of the right macroblock's
// partition 0 and of a 16x16 block) and 3 (v[1], neighbour A of its partition 2); both (0, 0) after P_Skip, an intra or I_PCM macroblock
// and at the start of a row - refIdx -1 or absent, which this slice layout never needs to tell from a zero vector (see the header).
struct h264_part_chain {
    int v[2][2];
};
H264_HD int h264_part_median(int a, int b, int c) { return a > b ? (b > c ? b : a > c ? c : a) : (a > c ? a : b > c ? c : b); }
// mvp of the four partitions from the chain and the macroblock's own vectors v[part][x / y] (partition i reads partitions < i only)
H264_HD void h264_part_mvp(const h264_part_chain& left, const int (*v)[2], int part, int* px, int* py) {
    if (part == 0) *px = left.v[0][0], *py = left.v[0][1];
    else if (part == 1) *px = v[0][0], *py = v[0][1];
    else if (part == 2) *px = h264_part_median(left.v[1][0], v[0][0], v[1][0]), *py = h264_part_median(left.v[1][1], v[0][1], v[1][1]);
    else *px = h264_part_median(v[2][0], v[1][0], v[0][0]), *py = h264_part_median(v[2][1], v[1][1], v[0][1]);
}
H264_HD bool h264_part_equal(const int (*v)[2]) {
    return v[1][0] == v[0][0] && v[2][0] == v[0][0] && v[3][0] == v[0][0] && v[1][1] == v[0][1] && v[2][1] == v[0][1] && v[3][1] == v[0][1];
}

// macroblock_layer() of a P_8x8 macroblock up to and including the luma residual: mb_type ue(3), four sub_mb_type ue(0) (P_L0_8x8), no
// ref_idx (one active reference), the four mvd_l0 pairs, coded_block_pattern by the inter column, mb_qp_delta only with cbp != 0
template <class Sink>
H264_HD void h264_part_code_inter(const int16_t* lev, int cbp_luma, int cbp_chroma, const h264_chain& left, const int (*mvd)[2], Sink& s, uint8_t* tcy) {
    h264_put_ue(s, 3u);                                 // mb_type P_8x8
    for (int i = 0; i < 4; ++i) h264_put_ue(s, 0u);     // sub_mb_type P_L0_8x8
    for (int i = 0; i < 4; ++i) h264_put_se(s, mvd[i][0]), h264_put_se(s, mvd[i][1]);
    h264_put_ue(s, (unsigned)h264_cbp_inter_code(cbp_luma + 16 * cbp_chroma));
    if (cbp_luma || cbp_chroma) h264_put_se(s, 0);      // mb_qp_delta
    for (int b = 0; b < 16; ++b) {
        if (!((cbp_luma >> (b >> 2)) & 1)) continue;
        const int bx = 2 * ((b >> 2) & 1) + (b & 1), by = 2 * (b >> 3) + ((b >> 1) & 1);
        const int a = bx ? tcy[by * 4 + bx - 1] : left.have ? left.tcy[by] : -1;
        const int t = by ? tcy[(by - 1) * 4 + bx] : -1;
        tcy[by * 4 + bx] = (uint8_t)h264_code_block(lev + (1 + b) * 16, 16, h264_nc(a, t), s);
    }
}
template <class Sink>
H264_HD void h264_part_code_mb(const int16_t* lev, int cbp_luma, int cbp_chroma, const h264_chain& left, const int (*mvd)[2], Sink& s, uint8_t* tcy,
                               uint8_t* tcc) {
    for (int i = 0; i < 16; ++i) tcy[i] = 0;            // [by * 4 + bx]
    for (int i = 0; i < 8; ++i) tcc[i] = 0;             // [c * 4 + by * 2 + bx]
    h264_part_code_inter(lev, cbp_luma, cbp_chroma, left, mvd, s, tcy);
    h264_gop_code_chroma(lev, cbp_chroma, left, s, tcc);
}

// serial: h264_gop_serial_sub with four vectors v[part] (quarter samples, already through h264_part_fetch; mb->fy / fc hold the
// per-partition prediction).  Four equal vectors, and every macroblock that is not inter, go through h264_gop_serial_sub itself with the
// chain's partition-1 vector as the predictor: today's bits.  Otherwise P_8x8; the counting pass includes its real syntax bits.
H264_HD void h264_gop_serial_part(h264_gop_mb* mb, unsigned nz, bool any_cdc, bool inter, bool p_slice, h264_chain& ch, h264_part_chain& pc,
                                  const int (*v)[2], h264_writer& w, int* skip_run) {
    if (!inter || h264_part_equal(v)) {
        h264_mv_chain mvc;
        mvc.vx = pc.v[0][0], mvc.vy = pc.v[0][1];
        h264_gop_serial_sub(mb, nz, any_cdc, inter, p_slice, ch, mvc, v[0][0], v[0][1], w, skip_run);
        pc.v[0][0] = pc.v[1][0] = mvc.vx, pc.v[0][1] = pc.v[1][1] = mvc.vy;
        return;
    }
    int cbp_luma = 0;
    for (int i = 0; i < 4; ++i)
        if (nz & (0xfu << (4 * i))) cbp_luma |= 1 << i;
    const int cbp_chroma = (nz & 0xff0000u) ? 2 : any_cdc ? 1 : 0;
    int mvd[4][2];
    for (int i = 0; i < 4; ++i) {
        int px, py;
        h264_part_mvp(pc, v, i, &px, &py);
        mvd[i][0] = v[i][0] - px, mvd[i][1] = v[i][1] - py;
    }
    h264_put_ue(w, (unsigned)*skip_run);                // mb_skip_run (P_8x8 exists in P slices only)
    *skip_run = 0;
    uint8_t tcy[16], tcc[8];
    h264_counter cnt;
    cnt.bits = 0, cnt.failed = false;
    h264_part_code_mb(mb->lev, cbp_luma, cbp_chroma, ch, mvd, cnt, tcy, tcc);
    if (cnt.failed || cnt.bits > 3200) {                // Annex A.3.1 / level_prefix <= 15: I_PCM
        h264_put_ue(w, 30u);
        while (w.n) w.put(0u, 1);                       // pcm_alignment_zero_bit
        for (int i = 0; i < 256; ++i) w.put(mb->sy[i], 8);
        for (int i = 0; i < 128; ++i) w.put(mb->sc[i], 8);
        for (int i = 0; i < 4; ++i) ch.tcy[i] = 16;
        ch.tcc[0][0] = ch.tcc[0][1] = ch.tcc[1][0] = ch.tcc[1][1] = 16;
        mb->mode = kH264ModePcm;
        pc.v[0][0] = pc.v[0][1] = pc.v[1][0] = pc.v[1][1] = 0;
        return;
    }
    h264_part_code_mb(mb->lev, cbp_luma, cbp_chroma, ch, mvd, w, tcy, tcc);
    for (int i = 0; i < 4; ++i) ch.tcy[i] = tcy[i * 4 + 3];
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 2; ++i) ch.tcc[c][i] = tcc[c * 4 + i * 2 + 1];
    mb->mode = kH264ModeInter;
    pc.v[0][0] = v[1][0], pc.v[0][1] = v[1][1], pc.v[1][0] = v[3][0], pc.v[1][1] = v[3][1];
}

// mbinfo word with four vectors: h264_lf_word (bit 18: all four coded vectors are (0, 0)) plus bits 19 .. 22 for an inter or skipped macroblock
H264_HD uint32_t h264_part_lf_word(int mode, unsigned nz, const int (*v)[2]) {
    uint32_t word = h264_lf_word(mode, nz, v[0][0] | v[1][0] | v[2][0] | v[3][0], v[0][1] | v[1][1] | v[2][1] | v[3][1]);
    if (!(word & (uint32_t)kH264LfIntra))
        for (int i = 0; i < 4; ++i)
            if (!v[i][0] && !v[i][1]) word |= (uint32_t)kH264LfZeroPart0 << i;
    return word;
}

// h264_gop_encode_mb_sub with four vectors: mb->sy / sc are loaded, and in a P picture the windows wy (4 x 13 x 13) and wc (2 x 4 x 5 x 5)
// through h264_part_luma_at / h264_part_chroma_at; leaves mb->ry / rc.  Returns the macroblock's side information word.  (Host; the
// kernel spreads the per-sample pieces over its lanes.)
inline uint32_t h264_gop_encode_mb_part(h264_gop_mb* mb, h264_chain& ch, h264_part_chain& pc, bool p_slice, int qp, const h264_sub_ref* at,
                                        const uint8_t* wy, const uint8_t* wc, h264_writer& w, int* skip_run) {
    int v[4][2];
    for (int i = 0; i < 4; ++i) v[i][0] = at[i].vx, v[i][1] = at[i].vy;
    if (p_slice) {
        for (int i = 0; i < 256; ++i) mb->fy[i] = (uint8_t)h264_part_pred_luma(wy, at, i & 15, i >> 4);
        for (int i = 0; i < 128; ++i)
            mb->fc[i] = (uint8_t)h264_part_pred_chroma(wc + (i >> 6) * 4 * kH264PartChromaWin * kH264PartChromaWin, at, i & 7, (i >> 3) & 7);
    }
    h264_gop_pred(mb, ch);
    bool inter = false;
    if (p_slice) {
        int si = 0, sp = 0;
        for (int b = 0; b < 16; ++b) {
            int a, c;
            h264_gop_block_sad(mb, b, &a, &c);
            si += a, sp += c;
        }
        inter = !(si < sp);
    }
    unsigned nz = 0;
    for (int b = 0; b < 24; ++b)
        if (h264_gop_block_forward(mb, b, inter, qp)) nz |= 1u << b;
    const bool any_cdc = h264_gop_dc(mb, inter, qp);
    h264_gop_serial_part(mb, nz, any_cdc, inter, p_slice, ch, pc, v, w, skip_run);
    const uint32_t word = h264_part_lf_word(mb->mode, nz, v);
    for (int b = 0; b < 24; ++b) h264_gop_block_recon(mb, b, qp);
    h264_gop_chain(mb, ch);
    return word;
}

// The search's decision: the four quadrant winners are taken iff sum cost8_q + 8 lambda < cost16(w16) (strict; 8 = the extra syntax bits
// of P_8x8 against P_L0_16x16).  Keys are h264_sub_key words.  out[part]: the vectors to write.
H264_HD bool h264_part_decide(const unsigned long long* key8, unsigned long long key16, int lambda, int (*out)[2]) {
    int c16, x16, y16, sum = 8 * lambda, q[4][2];
    h264_sub_unkey(key16, &c16, &x16, &y16);
    for (int i = 0; i < 4; ++i) {
        int c;
        h264_sub_unkey(key8[i], &c, &q[i][0], &q[i][1]);
        sum += c;
    }
    const bool take = sum < c16;
    for (int i = 0; i < 4; ++i) out[i][0] = take ? q[i][0] : x16, out[i][1] = take ? q[i][1] : y16;
    return take;
}

// One side of an edge with four vectors: the word and the partitions' vectors in quarter samples ((0, 0) for an intra macroblock, under
// bit 18, and for partition i under bit 19 + i).  ``v``: the macroblock's [4][2] of the mv tensor.
struct h264_part_side {
    uint32_t info;
    int v[4][2];
};
H264_HD h264_part_side h264_part_side_of(uint32_t info, const int16_t* v) {
    h264_part_side s;
    const bool zero = (info & (uint32_t)(kH264LfIntra | kH264LfZeroMv)) != 0;
    s.info = info;
    for (int i = 0; i < 4; ++i) {
        const bool z = zero || ((info >> (19 + i)) & 1u);
        s.v[i][0] = z ? 0 : (int)v[2 * i], s.v[i][1] = z ? 0 : (int)v[2 * i + 1];
    }
    return s;
}
H264_HD int h264_part_of_block(int blk) { return 2 * (blk >> 3) + ((blk >> 1) & 1); }   // blk = 4 by + bx
// h264_lf_bs with the vectors of the partitions that blocks pblk and qblk lie in
H264_HD int h264_part_bs(const h264_part_side& p, int pblk, const h264_part_side& q, int qblk, bool mb_edge) {
    if ((p.info | q.info) & (uint32_t)kH264LfIntra) return mb_edge ? 4 : 3;
    if (((p.info >> pblk) | (q.info >> qblk)) & 1u) return 2;
    const int* a = p.v[h264_part_of_block(pblk)];
    const int* b = q.v[h264_part_of_block(qblk)];
    const int dx = a[0] - b[0], dy = a[1] - b[1];
    return (dx >= 4 || dx <= -4 || dy >= 4 || dy <= -4) ? 1 : 0;
}
H264_HD int h264_part_index(const h264_part_side& p, const h264_part_side& q, int qp, bool chroma) {
    h264_lf_side a, b;
    a.info = p.info, b.info = q.info, a.vx = a.vy = b.vx = b.vy = 0;
    return h264_lf_index(a, b, qp, chroma);
}
// h264_lf_luma_line / h264_lf_chroma_line with four vectors a side
H264_HD void h264_part_luma_line(uint8_t* mb, int stride, int dir, int e, int l, const h264_part_side& p, const h264_part_side& q, int qp) {
    const int along = l >> 2, pe = e ? e - 1 : 3;
    const int qblk = dir ? 4 * e + along : 4 * along + e, pblk = dir ? 4 * pe + along : 4 * along + pe;
    const int bS = h264_part_bs(p, pblk, q, qblk, e == 0);
    if (!bS) return;
    h264_lf_line(dir ? mb + 4 * e * stride + l : mb + l * stride + 4 * e, dir ? stride : 1, bS, h264_part_index(p, q, qp, false), false);
}
H264_HD void h264_part_chroma_line(uint8_t* mb, int stride, int dir, int c, int l, const h264_part_side& p, const h264_part_side& q, int qp) {
    const int e = 2 * c, along = l >> 1, pe = e ? e - 1 : 3;
    const int qblk = dir ? 4 * e + along : 4 * along + e, pblk = dir ? 4 * pe + along : 4 * along + pe;
    const int bS = h264_part_bs(p, pblk, q, qblk, e == 0);
    if (!bS) return;
    h264_lf_line(dir ? mb + 4 * c * stride + l : mb + l * stride + 4 * c, dir ? stride : 1, bS, h264_part_index(p, q, qp, true), true);
}
// h264_lf_picture with four vectors a macroblock (host).  info [mbh * mbw], mv [mbh * mbw * 8].
inline void h264_part_lf_picture(uint8_t* ry, uint8_t* rcb, uint8_t* rcr, int mbh, int mbw, int qp, const uint32_t* info, const int16_t* mv) {
    const int lw = 16 * mbw, cw = 8 * mbw;
    for (int my = 0; my < mbh; ++my)
        for (int mx = 0; mx < mbw; ++mx) {
            const int at = my * mbw + mx;
            const h264_part_side q = h264_part_side_of(info[at], mv + 8 * at);
            const h264_part_side left = mx ? h264_part_side_of(info[at - 1], mv + 8 * (at - 1)) : q;
            const h264_part_side up = my ? h264_part_side_of(info[at - mbw], mv + 8 * (at - mbw)) : q;
            uint8_t* y0 = ry + (long long)my * 16 * lw + mx * 16;
            for (int dir = 0; dir < 2; ++dir)
                for (int e = 0; e < 4; ++e) {
                    if (e == 0 && !(dir ? my : mx)) continue;
                    for (int l = 0; l < 16; ++l) h264_part_luma_line(y0, lw, dir, e, l, e ? q : dir ? up : left, q, qp);
                }
            for (int c = 0; c < 2; ++c) {
                uint8_t* c0 = (c ? rcr : rcb) + (long long)my * 8 * cw + mx * 8;
                for (int dir = 0; dir < 2; ++dir)
                    for (int e = 0; e < 2; ++e) {
                        if (e == 0 && !(dir ? my : mx)) continue;
                        for (int l = 0; l < 8; ++l) h264_part_chroma_line(c0, cw, dir, e, l, e ? q : dir ? up : left, q, qp);
                    }
            }
        }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Row slices (sdv_hip_h264_seg.h "H.264 row slices"): every macroblock row is cut into ``segs`` slices of nearly equal width, each an
// independent bit stream with a wave of its own.  The pieces below are what the seg kernels, the host and the tests share: the number
// of slices a row gets, a slice's first and last macroblock, its slot index and the scratch layout - that of the intra layout at
// (n, mbh * segs, w'), so that sdv_h264_pack reads it unchanged.  Nothing above is touched.
// ------------------------------------------------------------------------------------------------------------------------------------
enum { kH264SegMax = 16 };                              // the largest row_slices setting
enum { kH264SegSlotRows = 1024 };                       // sdv_h264_pack accepts at most this many slot rows a picture
// slices actually written per row: the setting, at most one per macroblock, at most what sdv_h264_pack takes; the frame size alone decides
H264_HD int h264_row_segments(int mbh, int mbw, int row_slices) {
    int segs = row_slices < mbw ? row_slices : mbw;
    if (segs > kH264SegSlotRows / mbh) segs = kH264SegSlotRows / mbh;
    return segs < 1 ? 1 : segs;
}
// slice s of a row covers macroblocks h264_seg_first(s) .. h264_seg_first(s + 1) - 1: widths differ by at most one, none is empty (segs <= mbw)
H264_HD int h264_seg_first(int s, int mbw, int segs) { return (int)((long long)s * mbw / segs); }
H264_HD int h264_seg_width_max(int mbw, int segs) { return (mbw + segs - 1) / segs; }
// the slot of a slice is that of an intra picture this many macroblocks wide: h264_gop_slot_mbw of the widest slice
H264_HD int h264_seg_slot_mbw(int mbw, int segs) {
    const int w = h264_seg_width_max(mbw, segs);
    return w + 1 + w / 64;
}
H264_HD long long h264_seg_slot_index(long long f, int r, int s, int mbh, int segs) { return (f * mbh + r) * segs + s; }
// what the entry points accept: 1 .. min(mbw, 16) slices a row and at most 1024 slot rows a picture
H264_HD bool h264_seg_ok(int mbh, int mbw, int segs) {
    return segs >= 1 && segs <= kH264SegMax && segs <= mbw && (long long)mbh * segs <= kH264SegSlotRows;
}
struct h264_seg_layout {
    long long rows, slot, stride, starts_at, lens_at, bytes;
};
// the intra layout (sdv_hip.h "Capacity") at (n, mbh * segs, h264_seg_slot_mbw): slots at an 8-byte stride, an int64 start and an int32 length each
H264_HD h264_seg_layout h264_seg_scratch_layout(int n, int mbh, int mbw, int segs) {
    h264_seg_layout l;
    l.rows = (long long)n * mbh * segs;
    l.slot = 600LL * h264_seg_slot_mbw(mbw, segs) + 17;
    l.stride = (l.slot + 7) & ~7LL;
    l.starts_at = l.rows * l.stride;
    l.lens_at = l.starts_at + 8 * l.rows;
    l.bytes = l.lens_at + 4 * l.rows;
    return l;
}
H264_HD long long h264_seg_out_bytes(int n, int mbh, int mbw, int segs) { return (long long)n * mbh * segs * (600LL * h264_seg_slot_mbw(mbw, segs) + 17); }
