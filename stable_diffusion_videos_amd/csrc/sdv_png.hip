// PNG encoder (sdv_hip.h "PNG encoder"): uint8 RGB frames in HBM -> complete PNG files in one packed buffer.
//
//   sdv_png_filter_u8       frames -> filtered rows uint8 [n][H][1 + 3W] (libpng's minimum-sum-of-absolute-differences choice among the
//                           five filter types per row) and the per-row Adler-32 partials
//   sdv_png_deflate_pack    filtered rows -> signature | IHDR | one IDAT | IEND per frame, and offsets[n + 1]
//
// Stream: the zlib stream of a frame is `78 01`, then per STRIPE of stripe_rows filtered rows one dynamic-Huffman block (BFINAL 0,
// literals + end-of-block only, no matches; the code-length table is sent as plain 4-bit codes: HLIT 0, HDIST 0, HCLEN 15) followed by
// an empty stored block - which pads to a byte, so every stripe starts byte-aligned and the n * stripes stripes are independent bit
// streams: one wave each -, then `03 00` (a final fixed block that holds only end-of-block) and the Adler-32.  The IDAT CRC is left as
// a 4-byte hole of zeros: the host fills it from the bytes it copied back, or sdv_png_crc32 does in place.
//
//   sdv_png_deflate_lz_pack the same with LZ77 matches inside a stripe's block (opt-in; the rule is in sdv_hip.h "Matching mode")
//   sdv_png_crc32           the CRC-32 of every file's IDAT chunk, in place
#include "sdv_common.h"

namespace {

constexpr unsigned kAdlerMod = 65521u;
constexpr int kSyms = 257;                              // literals 0 .. 255 + end-of-block
constexpr int kMaxLen = 15;
constexpr int kTableBits = 3 + 14 + 19 * 3 + 258 * 4;   // block header + HLIT/HDIST/HCLEN + code-length code lengths + 257 + 1 lengths
constexpr int kPrefix = 33 + 8 + 2;                     // signature + IHDR | IDAT length + tag | 78 01
constexpr int kSuffix = 2 + 4 + 4 + 12;                 // 03 00 | Adler-32 | CRC hole | IEND
constexpr int kCodeWords = 260;                         // per stripe in the scratch: (length << 16 | bit-reversed code) [257], padded

// ---------------------------------------------------------------------------------------------------------------------------
// Filter.  One workgroup = one row.  Pass 1: every thread walks its bytes of the row once and sums the cost of each of the five filter
// types (sum of v < 128 ? v : 256 - v over the filtered bytes); the workgroup reduces the five sums and takes the minimum, ties to
// the lowest type.  Pass 2: the bytes again, filtered with the chosen type, stored (byte stores: a row of 1 + 3W bytes starts at any
// alignment) and summed into the row's Adler partials  A = sum d_j,  B = sum (R - j) d_j  (j = 0 .. R - 1, the type byte included),
// both mod 65521.  Filters read raw neighbours only (the row above is zeros for row 0), so rows are independent.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kFilterThreads = 256;

SDV_DEVICE unsigned filter_byte(int type, int x, int a, int b, int c) {
    int pred;
    switch (type) {
        case 0: pred = 0; break;
        case 1: pred = a; break;
        case 2: pred = b; break;
        case 3: pred = (a + b) >> 1; break;
        default: {
            const int p = a + b - c;
            const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
            pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
        }
    }
    return (unsigned)(x - pred) & 0xffu;
}
SDV_DEVICE unsigned msad(unsigned v) { return v < 128u ? v : 256u - v; }

template <class T>
SDV_DEVICE T wave_add(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(kFilterThreads) void png_filter_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ filtered,
                                                                    uint32_t* __restrict__ adler_rows, int H, int W) {
    __shared__ unsigned red[kFilterThreads / 64][5];
    __shared__ unsigned long long red2[kFilterThreads / 64][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long g = blockIdx.x;                     // row of the batch
    const int y = (int)(g % H);
    const int nb = 3 * W;
    const long long R = 1 + (long long)nb;
    const uint8_t* cur = frames + g * nb;
    const uint8_t* up = cur - nb;                       // (read only when y > 0)
    unsigned cost[5] = {0u, 0u, 0u, 0u, 0u};
    for (int i = tid; i < nb; i += kFilterThreads) {
        const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = y > 0 ? up[i] : 0, c = (y > 0 && i >= 3) ? up[i - 3] : 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) cost[t] += msad(filter_byte(t, x, a, b, c));
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const unsigned s = wave_add(cost[t]);
        if (lane == 0) red[wave][t] = s;
    }
    __syncthreads();
    int best = 0;
    unsigned best_cost = 0xffffffffu;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < kFilterThreads / 64; ++w) s += red[w][t];
        if (s < best_cost) best_cost = s, best = t;     // strict: ties stay with the lowest type
    }
    uint8_t* dst = filtered + g * R;
    unsigned long long A = 0, B = 0;
    if (tid == 0) {
        dst[0] = (uint8_t)best;
        A = (unsigned)best;
        B = (unsigned long long)R * (unsigned)best;
    }
    for (int i = tid; i < nb; i += kFilterThreads) {
        const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = y > 0 ? up[i] : 0, c = (y > 0 && i >= 3) ? up[i - 3] : 0;
        const unsigned v = filter_byte(best, x, a, b, c);
        dst[1 + i] = (uint8_t)v;
        A += v;
        B += (unsigned long long)(nb - i) * v;          // R - (1 + i)
    }
    A = wave_add(A);
    B = wave_add(B);
    if (lane == 0) red2[wave][0] = A, red2[wave][1] = B;
    __syncthreads();
    if (tid == 0) {
        unsigned long long a = 0, b = 0;
#pragma unroll
        for (int w = 0; w < kFilterThreads / 64; ++w) a += red2[w][0], b += red2[w][1];
        adler_rows[2 * g] = (uint32_t)(a % kAdlerMod);
        adler_rows[2 * g + 1] = (uint32_t)(b % kAdlerMod);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Reading a stripe.  A stripe is `len` consecutive bytes of the filtered buffer from an arbitrary byte address; lanes read it as
// aligned 32-bit words.  A word that is not wholly inside [lo, hi) - the first or the last of the whole buffer at most - is put
// together from byte loads of its bytes inside.
// ---------------------------------------------------------------------------------------------------------------------------
SDV_DEVICE unsigned load_word(const uint8_t* lo, const uint8_t* hi, const uint8_t* p) {
    if (p >= lo && p + 4 <= hi) return *(const unsigned*)p;
    unsigned v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (p + k >= lo && p + k < hi) v |= (unsigned)p[k] << (8 * k);
    return v;
}

SDV_DEVICE unsigned bit_reverse(unsigned code, int len) { return __brev(code) >> (32 - len); }

// ---------------------------------------------------------------------------------------------------------------------------
// Count.  One workgroup = one wave = one stripe:
//   1. histogram of the stripe's bytes in LDS (LDS atomic add), end-of-block counts 1;
//   2. the used symbols sorted by (count, symbol): every lane ranks its symbols against all 257 (LDS broadcast reads);
//   3. lane 0: Huffman tree by the two-queue merge over the sorted leaves, leaf depths, the number of codes per length with depths
//      beyond 15 folded into 15, then the Kraft sum brought back to 1 by moving one code at a time from the longest shorter length
//      down (the rule of miniz's tdefl_huffman_enforce_max_code_size: deterministic, keeps the code complete), lengths handed out
//      in sorted order - the rarest symbol gets the longest code.  When no leaf is deeper than 15 nothing moves and the cost is that
//      of the tree: the optimum;
//   4. lane 0: canonical codes (RFC 1951 3.2.2), stored bit-reversed;   5. the stripe's byte length.
// ---------------------------------------------------------------------------------------------------------------------------
// Workspace of one code: leaf weights ascending, internal node weights in the order they are made (ascending too), parents, depths.
template <int N>
struct HuffWs {
    unsigned lw[N], iw[N];
    unsigned short ssym[N], lpar[N], ipar[N], idepth[N];
    unsigned short cnt[kMaxLen + 1];
    int used;
};

// Steps 2 - 4 for the n <= N symbols of `hist` (LDS, complete): the whole wave calls it.  len8[n] receives the code lengths,
// ws.iw[1 .. 15] the first canonical code of every length.  One used symbol gets length 1 (the single incomplete code inflate
// accepts for distances), none leaves all lengths 0.
template <int N>
SDV_DEVICE void huffman_code(const unsigned* hist, int n, HuffWs<N>& ws, unsigned char* len8, int lane) {
    for (int i = lane; i < n; i += 64) len8[i] = 0;
    if (lane == 0) ws.used = 0;
    __syncthreads();
    for (int sym = lane; sym < n; sym += 64) {
        const unsigned c = hist[sym];
        if (c == 0) continue;
        int rank = 0;
        for (int t = 0; t < n; ++t) {
            const unsigned o = hist[t];
            rank += (o != 0 && (o < c || (o == c && t < sym))) ? 1 : 0;
        }
        ws.ssym[rank] = (unsigned short)sym;
        ws.lw[rank] = c;
        atomicAdd(&ws.used, 1);
    }
    __syncthreads();
    if (lane == 0) {
        const int m = ws.used;
        for (int i = 0; i <= kMaxLen; ++i) ws.cnt[i] = 0;
        if (m == 1) ws.cnt[1] = 1;
        if (m >= 2) {
            int li = 0, ii = 0;
            for (int k = 0; k < m - 1; ++k) {           // internal node k takes the two lightest of what is left; a leaf wins a tie
                unsigned w = 0;
                for (int t = 0; t < 2; ++t) {
                    if (li < m && (ii >= k || ws.lw[li] <= ws.iw[ii])) {
                        w += ws.lw[li];
                        ws.lpar[li++] = (unsigned short)k;
                    } else {
                        w += ws.iw[ii];
                        ws.ipar[ii++] = (unsigned short)k;
                    }
                }
                ws.iw[k] = w;
            }
            ws.idepth[m - 2] = 0;
            for (int k = m - 3; k >= 0; --k) ws.idepth[k] = (unsigned short)(ws.idepth[ws.ipar[k]] + 1);
            for (int i = 0; i < m; ++i) {
                const int d = ws.idepth[ws.lpar[i]] + 1;
                ++ws.cnt[d < kMaxLen ? d : kMaxLen];
            }
            unsigned kraft = 0;
            for (int i = 1; i <= kMaxLen; ++i) kraft += (unsigned)ws.cnt[i] << (kMaxLen - i);
            while (kraft > (1u << kMaxLen)) {
                --ws.cnt[kMaxLen];
                for (int i = kMaxLen - 1; i > 0; --i)
                    if (ws.cnt[i]) {
                        --ws.cnt[i];
                        ws.cnt[i + 1] += 2;
                        break;
                    }
                --kraft;
            }
        }
        int at = 0;
        for (int l = kMaxLen; l >= 1; --l)
            for (int c = ws.cnt[l]; c > 0; --c) len8[ws.ssym[at++]] = (unsigned char)l;
        // canonical codes: the first of every length (indexed by a runtime length later: kept in LDS - iw is dead from here on)
        unsigned code = 0;
        for (int l = 1; l <= kMaxLen; ++l) {
            code = (code + (l > 1 ? ws.cnt[l - 1] : 0u)) << 1;
            ws.iw[l] = code;
        }
    }
    __syncthreads();
}

// a symbol's code word for the write stage: length << 16 | bit-reversed (first code of its length + the number of smaller symbols
// with that length); 0 for an unused symbol
SDV_DEVICE unsigned code_entry(const unsigned char* len8, const unsigned* first, int sym) {
    const int l = len8[sym];
    if (!l) return 0u;
    unsigned before = 0;
    for (int t = 0; t < sym; ++t) before += len8[t] == l ? 1u : 0u;
    return ((unsigned)l << 16) | bit_reverse(first[l] + before, l);
}

__global__ __launch_bounds__(64) void png_count_kernel(const uint8_t* __restrict__ filtered, long long total_bytes, int H, long long R,
                                                       int stripe_rows, int stripes, long long* __restrict__ lens,
                                                       uint32_t* __restrict__ codes, uint8_t* __restrict__ lengths) {
    __shared__ unsigned hist[kSyms];
    __shared__ HuffWs<kSyms> ws;
    __shared__ unsigned char len8[kSyms];
    const int lane = threadIdx.x;
    const long long stripe = blockIdx.x;
    const int s = (int)(stripe % stripes);
    const long long f = stripe / stripes;
    const int row0 = s * stripe_rows, rows = min(stripe_rows, H - row0);
    const long long start = (f * H + row0) * R, len = (long long)rows * R;
    for (int i = lane; i < kSyms; i += 64) hist[i] = i == 256 ? 1u : 0u;
    __syncthreads();
    {
        const uint8_t* lo = filtered;
        const uint8_t* hi = filtered + total_bytes;
        const uint8_t* p0 = filtered + start;
        const int sh = (int)((uintptr_t)p0 & 3);
        const uint8_t* a0 = p0 - sh;
        const long long nwords = (sh + len + 3) >> 2;
        for (long long w = lane; w < nwords; w += 64) {
            const unsigned v = load_word(lo, hi, a0 + 4 * w);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long j = 4 * w + k - sh;     // byte of the stripe
                if (j >= 0 && j < len) atomicAdd(&hist[(v >> (8 * k)) & 0xffu], 1u);
            }
        }
    }
    __syncthreads();
    huffman_code(hist, kSyms, ws, len8, lane);          // (at least two symbols here: end-of-block and one literal)
    unsigned long long bits = 0;
    uint32_t* my_codes = codes + stripe * kCodeWords;
    for (int sym = lane; sym < kCodeWords; sym += 64) {
        unsigned entry = 0;
        if (sym < kSyms) {
            entry = code_entry(len8, ws.iw, sym);
            bits += (unsigned long long)hist[sym] * (entry >> 16);
            if (lengths) lengths[stripe * kSyms + sym] = len8[sym];
        }
        my_codes[sym] = entry;
    }
    bits = wave_add(bits);
    // table + data (end-of-block included) + the stored block's 3 header bits, padded to a byte, + 00 00 FF FF
    if (lane == 0) lens[stripe] = (long long)((kTableBits + bits + 3 + 7) >> 3) + 4;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Scan.  ONE workgroup: exclusive scan of the stripe lengths, frame-major, with the 43 bytes in front of every frame's first stripe and
// the 22 behind its last -> starts[stripe], offsets[frame], offsets[n] = *needed; then the Adler-32 of every frame from its rows'
// partials:  a = 1 + sum A_r,  b = H R + sum (B_r + (H - 1 - r) R A_r)   (mod 65521).
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kScanThreads = 256;

__global__ __launch_bounds__(kScanThreads) void png_scan_kernel(const long long* __restrict__ lens, long long* __restrict__ starts,
                                                                long long n_stripes, int stripes, int n, int H, long long R,
                                                                const uint32_t* __restrict__ adler_rows, uint32_t* __restrict__ adlers,
                                                                long long* __restrict__ offsets, long long* __restrict__ needed) {
    __shared__ long long wsum[kScanThreads / 64];
    __shared__ long long running;
    __shared__ unsigned long long asum[kScanThreads / 64][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) running = 0;
    __syncthreads();
    for (long long i0 = 0; i0 < n_stripes; i0 += kScanThreads) {
        const long long i = i0 + tid;
        const long long mine = i < n_stripes ? lens[i] : 0;
        long long incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long upv = __shfl_up(incl, o);
            if (lane >= o) incl += upv;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        long long before = running;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (i < n_stripes) {
            const long long f = i / stripes;
            const long long first = before + incl - mine + f * (kPrefix + kSuffix) + kPrefix;
            starts[i] = first;
            if (i % stripes == 0) offsets[f] = first - kPrefix;
        }
        __syncthreads();
        if (tid == kScanThreads - 1) running = before + incl;
        __syncthreads();
    }
    if (tid == 0) {
        const long long total = running + (long long)n * (kPrefix + kSuffix);
        offsets[n] = total;
        *needed = total;
    }
    const unsigned long long Rm = (unsigned long long)(R % kAdlerMod);
    for (int f = 0; f < n; ++f) {
        unsigned long long a = 0, b = 0;
        for (int r = tid; r < H; r += kScanThreads) {
            const unsigned long long A = adler_rows[2 * ((long long)f * H + r)], B = adler_rows[2 * ((long long)f * H + r) + 1];
            const unsigned long long below = ((unsigned long long)(H - 1 - r) % kAdlerMod) * Rm % kAdlerMod;
            a += A;                                     // < 2^16 each, H <= 16384
            b += (B + below * A) % kAdlerMod;
        }
        a = wave_add(a);
        b = wave_add(b);
        __syncthreads();
        if (lane == 0) asum[wave][0] = a, asum[wave][1] = b;
        __syncthreads();
        if (tid == 0) {
            a = 1, b = ((unsigned long long)H % kAdlerMod) * Rm;
            for (int w = 0; w < kScanThreads / 64; ++w) a += asum[w][0], b += asum[w][1];
            adlers[f] = (uint32_t)(((b % kAdlerMod) << 16) | (a % kAdlerMod));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Write.  One workgroup = one wave = one stripe, storing at the stripe's final position in `out`.  The bit stream is LSB-first, so a
// buffer of 32-bit words in LDS that bits are OR-ed into (bit i of the stream = bit i & 31 of word i >> 5) IS the byte stream.
//   table:  the 1106 bits of block header and code lengths; 138 whole bytes leave, 2 bits open the first data pass;
//   data:   passes of 1024 bytes: the bytes are staged in LDS (aligned word loads), every lane takes 16 consecutive ones, sums their
//           code lengths, the wave's exclusive prefix sum is the lane's bit position, the lane ORs its codes in (LDS atomic OR:
//           neighbours share a word); the whole bytes leave, the up to 7 bits left over open the next pass;
//   end:    end-of-block, the empty stored block (000, pad, 00 00 FF FF).
// The wave of a frame's first stripe also stores the 43 bytes in front, the wave of its last stripe the 22 behind.
// No store is issued at or beyond out_cap, and none at all when *needed > out_cap.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kPassBytes = 1024, kLaneBytes = kPassBytes / 64;
constexpr int kBitWords = (7 + kPassBytes * kMaxLen + 31) / 32 + 4;

SDV_DEVICE void put_byte(uint8_t* out, long long cap, long long at, unsigned v) {
    if (at >= 0 && at < cap) out[at] = (uint8_t)v;
}

// nbytes bytes of the LDS words `buf` -> out[at ..): bytes up to the first 4-byte aligned address, then 32-bit stores, then bytes
SDV_DEVICE void flush_bytes(uint8_t* out, long long cap, long long at, const unsigned* buf, int nbytes, int lane) {
    const uint8_t* b8 = (const uint8_t*)buf;
    int head = (int)((4 - (((uintptr_t)out + (unsigned long long)at) & 3)) & 3);
    head = min(head, nbytes);
    if (lane < head) put_byte(out, cap, at + lane, b8[lane]);
    const int nw = (nbytes - head) >> 2;
    const int sh = 8 * (head & 3);
    for (int j = lane; j < nw; j += 64) {
        const int src = head + 4 * j;
        const unsigned lo = buf[src >> 2], hi = buf[(src >> 2) + 1];
        const unsigned v = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
        const long long p = at + src;
        if (p + 4 <= cap) *(unsigned*)(out + p) = v;
    }
    const int done = head + 4 * nw;
    if (lane < nbytes - done) put_byte(out, cap, at + done + lane, b8[done + lane]);
}

// the 43 bytes in front of a frame's first stripe (which starts at `at`), the 22 behind its last (which ends at `end`)
SDV_DEVICE void put_file_ends(uint8_t* out, long long out_cap, int s, int stripes, long long f, long long at, long long end,
                              const uint32_t* adlers, const uint8_t* header, const long long* offsets, int lane) {
    if (s == 0) {
        const long long idat = offsets[f + 1] - offsets[f] - (kPrefix + kSuffix) + 2 + 2 + 4;      // 78 01 | stripes | 03 00 | Adler-32
        if (lane < 33) put_byte(out, out_cap, at - kPrefix + lane, header[lane]);
        if (lane < 4) put_byte(out, out_cap, at - 10 + lane, (unsigned)(idat >> (24 - 8 * lane)) & 0xffu);
        if (lane >= 4 && lane < 10) {
            const unsigned char tag[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
            put_byte(out, out_cap, at - 10 + lane, tag[lane - 4]);
        }
    }
    if (s == stripes - 1 && lane < kSuffix) {
        const unsigned ad = adlers[f];
        const unsigned char tail[kSuffix] = {0x03, 0x00, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
        unsigned v = tail[lane];
        if (lane >= 2 && lane < 6) v = (ad >> (24 - 8 * (lane - 2))) & 0xffu;
        put_byte(out, out_cap, end + lane, v);
    }
}

// tok_counts: NULL, or the token count of every stripe (matching mode): a stripe with fewer tokens than bytes holds matches and is
// png_lz_write_kernel's.
__global__ __launch_bounds__(64) void png_write_kernel(const uint8_t* __restrict__ filtered, long long total_bytes, int H, long long R,
                                                       int stripe_rows, int stripes, const long long* __restrict__ starts,
                                                       const long long* __restrict__ lens, const uint32_t* __restrict__ codes,
                                                       const uint32_t* __restrict__ adlers, const uint8_t* __restrict__ header,
                                                       const long long* __restrict__ offsets, uint8_t* __restrict__ out,
                                                       long long out_cap, const long long* __restrict__ needed,
                                                       const uint32_t* __restrict__ tok_counts) {
    __shared__ unsigned bits[kBitWords];
    __shared__ unsigned code[kCodeWords];
    __shared__ unsigned inw[kPassBytes / 4 + 2];
    if (*needed > out_cap) return;                      // the host retries with a buffer of *needed bytes: nothing is written
    const int lane = threadIdx.x;
    const long long stripe = blockIdx.x;
    const int s = (int)(stripe % stripes);
    const long long f = stripe / stripes;
    const int row0 = s * stripe_rows, rows = min(stripe_rows, H - row0);
    const long long start = (f * H + row0) * R, len = (long long)rows * R;
    if (tok_counts && (long long)tok_counts[stripe] != len) return;
    long long at = starts[stripe];
    put_file_ends(out, out_cap, s, stripes, f, at, at + lens[stripe], adlers, header, offsets, lane);
    for (int i = lane; i < kCodeWords; i += 64) code[i] = codes[stripe * kCodeWords + i];
    for (int i = lane; i < kBitWords; i += 64) bits[i] = 0u;
    __syncthreads();
    // ---- table: BFINAL 0, BTYPE 10b, HLIT 0, HDIST 0, HCLEN 15, sixteen 3-bit fields: 0 0 0 then 4 x 16, 258 lengths as 4-bit codes
    if (lane == 0) {
        atomicOr(&bits[0], (2u << 1) | (15u << 13));                             // bits 0 .. 16
        // code-length code lengths from bit 17: symbols 16, 17, 18 get 0 (9 bits), then sixteen times 4 (bit 2 of each field)
        for (int k = 3; k < 19; ++k) {
            const int p = 17 + 3 * k + 2;
            atomicOr(&bits[p >> 5], 1u << (p & 31));
        }
    }
    for (int k = lane; k < 258; k += 64) {
        const unsigned l = k < kSyms ? code[k] >> 16 : 0u;                         // (k = 257: the one distance code, length 0)
        const int p = 74 + 4 * k;                                                // p & 31 = 30: the nibble straddles two words
        const unsigned nib = bit_reverse(l, 4);
        atomicOr(&bits[p >> 5], nib << (p & 31));
        if ((p & 31) > 28) atomicOr(&bits[(p >> 5) + 1], nib >> (32 - (p & 31)));
    }
    __syncthreads();
    flush_bytes(out, out_cap, at, bits, kTableBits >> 3, lane);
    at += kTableBits >> 3;
    unsigned carry = kTableBits & 7;
    unsigned last = (bits[(kTableBits >> 3) >> 2] >> (8 * ((kTableBits >> 3) & 3))) & ((1u << carry) - 1u);
    __syncthreads();
    for (int i = lane; i < kBitWords; i += 64) bits[i] = i == 0 ? last : 0u;
    __syncthreads();
    // ---- data
    const uint8_t* lo = filtered;
    const uint8_t* hi = filtered + total_bytes;
    for (long long c0 = 0; c0 < len; c0 += kPassBytes) {
        const int cn = (int)min((long long)kPassBytes, len - c0);
        const uint8_t* p0 = filtered + start + c0;
        const int sh = (int)((uintptr_t)p0 & 3);
        const int nwords = (sh + cn + 3) >> 2;
        for (int w = lane; w < nwords; w += 64) inw[w] = load_word(lo, hi, p0 - sh + 4 * w);
        __syncthreads();
        const uint8_t* mine = (const uint8_t*)inw + sh + lane * kLaneBytes;
        const int cnt = max(0, min(kLaneBytes, cn - lane * kLaneBytes));
        unsigned nbits = 0;
        for (int k = 0; k < cnt; ++k) nbits += code[mine[k]] >> 16;
        unsigned incl = nbits;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned upv = __shfl_up(incl, o);
            if (lane >= o) incl += upv;
        }
        const unsigned pass_bits = carry + __shfl(incl, 63);
        {
            const unsigned pos = carry + incl - nbits;
            unsigned word = pos >> 5;
            int nb = (int)(pos & 31);
            unsigned long long acc = 0;
            for (int k = 0; k < cnt; ++k) {
                const unsigned e = code[mine[k]];
                acc |= (unsigned long long)(e & 0xffffu) << nb;
                nb += (int)(e >> 16);
                if (nb >= 32) {
                    atomicOr(&bits[word], (unsigned)acc);
                    ++word;
                    acc >>= 32;
                    nb -= 32;
                }
            }
            if (nb > 0 && acc) atomicOr(&bits[word], (unsigned)acc);
        }
        __syncthreads();
        const int nbytes = (int)(pass_bits >> 3);
        flush_bytes(out, out_cap, at, bits, nbytes, lane);
        at += nbytes;
        carry = pass_bits & 7u;
        last = (bits[nbytes >> 2] >> (8 * (nbytes & 3))) & ((1u << carry) - 1u);
        __syncthreads();
        for (unsigned i = lane; i <= (pass_bits >> 5) + 1 && i < (unsigned)kBitWords; i += 64) bits[i] = i == 0 ? last : 0u;
        __syncthreads();
    }
    // ---- end-of-block | 000 | pad | 00 00 FF FF
    const unsigned eob = code[256];
    const unsigned end_bits = carry + (eob >> 16) + 3;
    const int end_bytes = (int)((end_bits + 7) >> 3);   // <= 4
    if (lane == 0) {
        const unsigned long long v = (unsigned long long)bits[0] | ((unsigned long long)(eob & 0xffffu) << carry) |
                                     (0xffff0000ull << (8 * end_bytes));
        bits[0] = (unsigned)v;
        bits[1] = (unsigned)(v >> 32);
        bits[2] = 0u;
    }
    __syncthreads();
    flush_bytes(out, out_cap, at, bits, end_bytes + 4, lane);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Matches (sdv_hip.h "matching mode").  Token: len << 16 | dist for a match, the byte for a literal.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kLlSyms = 286, kDSyms = 30;               // literal / length symbols, distance symbols
constexpr int kLzCodeWords = 320;                       // per stripe: 286 literal / length code words, 30 distance code words, padded
constexpr int kLzTableBits = 3 + 14 + 19 * 3 + (kLlSyms + kDSyms) * 4;
constexpr int kHashSize = 4096, kGroup = 64, kMaxDist = 32768, kMaxMatch = 258;

// RFC 1951 3.2.5: symbol and number of extra bits of a length 3 .. 258 / a distance 1 .. 32768 (the extra value is the low bits of
// len - 3 / dist - 1)
SDV_DEVICE int len_symbol(int len, int& extra) {
    const int l = len - 3;
    extra = 0;
    if (len == kMaxMatch) return 285;
    if (l < 8) return 257 + l;
    extra = 29 - __clz(l);                              // floor(log2 l) - 2
    return 257 + 4 * (extra + 1) + ((l >> extra) & 3);
}
SDV_DEVICE int dist_symbol(int dist, int& extra) {
    const int x = dist - 1;
    extra = 0;
    if (x < 4) return x;
    const int nb = 31 - __clz(x);
    extra = nb - 1;
    return 2 * nb + ((x >> extra) & 1);
}

SDV_DEVICE unsigned hash3(const uint8_t* p) {
    const unsigned v = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
    return (v * 0x9E3779B1u) >> 20;
}

// common prefix of a[0 .. cap) and b[0 .. cap), b < a (the two may overlap): words while four bytes are left, then bytes - no
// byte at or beyond a + cap is read
SDV_DEVICE int match_length(const uint8_t* a, const uint8_t* b, int cap) {
    int k = 0;
    while (k + 4 <= cap) {
        unsigned x, y;
        __builtin_memcpy(&x, a + k, 4);
        __builtin_memcpy(&y, b + k, 4);
        const unsigned diff = x ^ y;
        if (diff) return k + (__builtin_ctz(diff) >> 3);
        k += 4;
    }
    while (k < cap && a[k] == b[k]) ++k;
    return k;
}

// Match.  One workgroup = one wave = one stripe, in groups of 64 positions.  Per group: every lane at or behind the parse cursor
// looks at its position's nine candidates (eight fixed distances and the head table's entry, which holds positions of EARLIER
// groups only) and prices its best match against the literal code of the count stage; the wave then walks the greedy path through
// the group (one cross-lane read per step), the lanes on the path store their tokens; last, the group's positions enter the head
// table (LDS atomic max: the largest position wins, whatever the order).  A group that lies inside an accepted match only enters
// the table.
__global__ __launch_bounds__(64) void png_match_kernel(const uint8_t* __restrict__ filtered, int H, long long R, int stripe_rows, int stripes,
                                                       const uint32_t* __restrict__ codes, uint32_t* __restrict__ tokens,
                                                       uint32_t* __restrict__ tok_counts) {
    __shared__ int head[kHashSize];
    __shared__ unsigned char price[kSyms];
    const int lane = threadIdx.x;
    const long long stripe = blockIdx.x;
    const int s = (int)(stripe % stripes);
    const long long f = stripe / stripes;
    const int row0 = s * stripe_rows, rows = min(stripe_rows, H - row0);
    const long long start = (f * H + row0) * R;
    const int L = (int)((long long)rows * R);           // <= 16384 * 49153 < 2^31
    const uint8_t* src = filtered + start;
    uint32_t* tok = tokens + start;
    for (int i = lane; i < kHashSize; i += 64) head[i] = -1;
    for (int i = lane; i < kSyms; i += 64) price[i] = (unsigned char)(codes[stripe * kCodeWords + i] >> 16);
    __syncthreads();
    const int Ri = (int)R;
    const int fixed[8] = {1, 2, 3, 4, 6, Ri - 3, Ri, Ri + 3};
    int cursor = 0, ntok = 0;
    for (int base = 0; base < L; base += kGroup) {
        const int i = base + lane;
        const bool hashed = i + 3 <= L;
        const unsigned h = hashed ? hash3(src + i) : 0u;
        if (cursor < base + kGroup) {
            int mlen = 0, mdist = 0;
            if (i >= cursor && hashed) {
                const int cap = min(kMaxMatch, L - i);
                const int j = head[h];
                int best = 0, bd = 0;
#pragma unroll 1
                for (int c = 0; c < 9; ++c) {
                    const int d = c < 8 ? fixed[c] : (j >= 0 ? i - j : 0);
                    if (d < 1 || d > i || d > kMaxDist) continue;
                    const int l = match_length(src + i, src + i - d, cap);
                    if (l > best || (l == best && d < bd)) best = l, bd = d;
                }
                if (best >= 3) {
                    int el, ed;
                    len_symbol(best, el);
                    dist_symbol(bd, ed);
                    const int limit = 12 + el + ed;
                    int sum = 0;
                    for (int k = 0; k < best && sum <= limit; ++k) sum += price[src[i + k]];
                    if (sum > limit) mlen = best, mdist = bd;
                }
            }
            unsigned long long path = 0;
            int p = cursor;
            while (p < base + kGroup && p < L) {
                const int l = __shfl(mlen, p - base);
                path |= 1ull << (p - base);
                p += l ? l : 1;
            }
            cursor = p;
            if ((path >> lane) & 1ull) {
                const int idx = ntok + __popcll(path & ((1ull << lane) - 1ull));
                tok[idx] = mlen ? ((unsigned)mlen << 16) | (unsigned)mdist : (unsigned)src[i];
            }
            ntok += __popcll(path);
        }
        __syncthreads();
        if (hashed) atomicMax(&head[h], i);
        __syncthreads();
    }
    if (lane == 0) tok_counts[stripe] = (uint32_t)ntok;
}

// Count for token streams.  One wave = one stripe.  A stripe without a match keeps the count stage's code and byte length.  Else:
// histograms of the tokens over the 286 literal / length symbols (end-of-block counts 1) and the 30 distance symbols, the two
// codes by the same builder, the code words, and the stripe's byte length with the 168-byte table.
__global__ __launch_bounds__(64) void png_lz_count_kernel(int H, long long R, int stripe_rows, int stripes, const uint32_t* __restrict__ tokens,
                                                          const uint32_t* __restrict__ tok_counts, const uint32_t* __restrict__ codes,
                                                          uint32_t* __restrict__ lz_codes, long long* __restrict__ lens,
                                                          uint8_t* __restrict__ ll_lengths, uint8_t* __restrict__ d_lengths) {
    __shared__ unsigned hist[kLlSyms + kDSyms];
    __shared__ HuffWs<kLlSyms> ws;
    __shared__ unsigned char len8[kLlSyms + kDSyms];
    const int lane = threadIdx.x;
    const long long stripe = blockIdx.x;
    const int s = (int)(stripe % stripes);
    const long long f = stripe / stripes;
    const int row0 = s * stripe_rows, rows = min(stripe_rows, H - row0);
    const long long start = (f * H + row0) * R, len = (long long)rows * R;
    const long long ntok = tok_counts[stripe];
    if (ntok == len) {                                  // no match: the literal code, no distance code
        for (int i = lane; i < kLlSyms; i += 64)
            if (ll_lengths) ll_lengths[stripe * kLlSyms + i] = i < kSyms ? (uint8_t)(codes[stripe * kCodeWords + i] >> 16) : (uint8_t)0;
        if (d_lengths && lane < kDSyms) d_lengths[stripe * kDSyms + lane] = 0;
        return;
    }
    for (int i = lane; i < kLlSyms + kDSyms; i += 64) hist[i] = i == 256 ? 1u : 0u;
    __syncthreads();
    const uint32_t* tok = tokens + start;
    unsigned long long bits = 0;
    for (long long k = lane; k < ntok; k += 64) {
        const unsigned t = tok[k];
        if (t >> 16) {
            int el, ed;
            atomicAdd(&hist[len_symbol((int)(t >> 16), el)], 1u);
            atomicAdd(&hist[kLlSyms + dist_symbol((int)(t & 0xffffu), ed)], 1u);
            bits += (unsigned)(el + ed);
        } else {
            atomicAdd(&hist[t], 1u);
        }
    }
    __syncthreads();
    uint32_t* my_codes = lz_codes + stripe * kLzCodeWords;
    huffman_code(hist, kLlSyms, ws, len8, lane);
    for (int sym = lane; sym < kLlSyms; sym += 64) {
        const unsigned entry = code_entry(len8, ws.iw, sym);
        bits += (unsigned long long)hist[sym] * (entry >> 16);
        my_codes[sym] = entry;
        if (ll_lengths) ll_lengths[stripe * kLlSyms + sym] = len8[sym];
    }
    __syncthreads();
    huffman_code(hist + kLlSyms, kDSyms, ws, len8 + kLlSyms, lane);
    for (int sym = lane; sym < kLzCodeWords - kLlSyms; sym += 64) {
        unsigned entry = 0;
        if (sym < kDSyms) {
            entry = code_entry(len8 + kLlSyms, ws.iw, sym);
            bits += (unsigned long long)hist[kLlSyms + sym] * (entry >> 16);
            if (d_lengths) d_lengths[stripe * kDSyms + sym] = len8[kLlSyms + sym];
        }
        my_codes[kLlSyms + sym] = entry;
    }
    bits = wave_add(bits);
    if (lane == 0) lens[stripe] = (long long)((kLzTableBits + bits + 3 + 7) >> 3) + 4;
}

// Write for token streams.  One wave = one stripe that holds a match (the others are png_write_kernel's), the same skeleton:
//   table:  the 1338 bits of block header (HLIT 29, HDIST 29, HCLEN 15) and 286 + 30 code lengths; 167 whole bytes leave;
//   data:   passes of 512 tokens read from HBM: every lane takes 8 consecutive ones, sums their bit lengths (code + extra bits of
//           the length, code + extra bits of the distance: at most 48 a token), the wave's exclusive prefix sum is the lane's bit
//           position, the lane ORs its bits in; whole bytes leave, the bits left over open the next pass;
//   end:    end-of-block, the empty stored block.
constexpr int kPassTokens = 512, kLaneTokens = kPassTokens / 64;
constexpr int kLzBitWords = (7 + kPassTokens * 48 + 31) / 32 + 4;
static_assert(kLzBitWords * 32 >= kLzTableBits + 64, "the table is put together in the same buffer");

// the bits of one token: piece 0 = literal code, or length code + extra bits; piece 1 = distance code + extra bits (or nothing)
SDV_DEVICE void token_bits(unsigned t, const unsigned* code, unsigned& v0, int& n0, unsigned& v1, int& n1) {
    if (t >> 16) {
        int e;
        const int len = (int)(t >> 16), dist = (int)(t & 0xffffu);
        unsigned ce = code[len_symbol(len, e)];
        int cl = (int)(ce >> 16);
        v0 = (ce & 0xffffu) | (((unsigned)(len - 3) & ((1u << e) - 1u)) << cl);
        n0 = cl + e;
        ce = code[kLlSyms + dist_symbol(dist, e)];
        cl = (int)(ce >> 16);
        v1 = (ce & 0xffffu) | (((unsigned)(dist - 1) & ((1u << e) - 1u)) << cl);
        n1 = cl + e;
    } else {
        const unsigned ce = code[t];
        v0 = ce & 0xffffu;
        n0 = (int)(ce >> 16);
        v1 = 0u;
        n1 = 0;
    }
}

__global__ __launch_bounds__(64) void png_lz_write_kernel(int H, long long R, int stripe_rows, int stripes, const uint32_t* __restrict__ tokens,
                                                          const uint32_t* __restrict__ tok_counts, const long long* __restrict__ starts,
                                                          const long long* __restrict__ lens, const uint32_t* __restrict__ lz_codes,
                                                          const uint32_t* __restrict__ adlers, const uint8_t* __restrict__ header,
                                                          const long long* __restrict__ offsets, uint8_t* __restrict__ out,
                                                          long long out_cap, const long long* __restrict__ needed) {
    __shared__ unsigned bits[kLzBitWords];
    __shared__ unsigned code[kLzCodeWords];
    if (*needed > out_cap) return;
    const int lane = threadIdx.x;
    const long long stripe = blockIdx.x;
    const int s = (int)(stripe % stripes);
    const long long f = stripe / stripes;
    const int row0 = s * stripe_rows, rows = min(stripe_rows, H - row0);
    const long long start = (f * H + row0) * R, len = (long long)rows * R;
    const long long ntok = tok_counts[stripe];
    if (ntok == len) return;
    const uint32_t* tok = tokens + start;
    long long at = starts[stripe];
    put_file_ends(out, out_cap, s, stripes, f, at, at + lens[stripe], adlers, header, offsets, lane);
    for (int i = lane; i < kLzCodeWords; i += 64) code[i] = lz_codes[stripe * kLzCodeWords + i];
    for (int i = lane; i < kLzBitWords; i += 64) bits[i] = 0u;
    __syncthreads();
    // ---- table: BFINAL 0, BTYPE 10b, HLIT 29, HDIST 29, HCLEN 15, the same nineteen 3-bit fields, 316 lengths as 4-bit codes
    if (lane == 0) {
        atomicOr(&bits[0], (2u << 1) | (29u << 3) | (29u << 8) | (15u << 13));
        for (int k = 3; k < 19; ++k) {
            const int p = 17 + 3 * k + 2;
            atomicOr(&bits[p >> 5], 1u << (p & 31));
        }
    }
    for (int k = lane; k < kLlSyms + kDSyms; k += 64) {
        const unsigned l = code[k] >> 16;
        const int p = 74 + 4 * k;
        const unsigned nib = bit_reverse(l, 4);
        atomicOr(&bits[p >> 5], nib << (p & 31));
        if ((p & 31) > 28) atomicOr(&bits[(p >> 5) + 1], nib >> (32 - (p & 31)));
    }
    __syncthreads();
    flush_bytes(out, out_cap, at, bits, kLzTableBits >> 3, lane);
    at += kLzTableBits >> 3;
    unsigned carry = kLzTableBits & 7;
    unsigned last = (bits[(kLzTableBits >> 3) >> 2] >> (8 * ((kLzTableBits >> 3) & 3))) & ((1u << carry) - 1u);
    __syncthreads();
    for (int i = lane; i < kLzBitWords; i += 64) bits[i] = i == 0 ? last : 0u;
    __syncthreads();
    // ---- data
    for (long long c0 = 0; c0 < ntok; c0 += kPassTokens) {
        const long long first = c0 + (long long)lane * kLaneTokens;
        const int cnt = (int)max(0LL, min((long long)kLaneTokens, ntok - first));
        unsigned mine[kLaneTokens];
#pragma unroll
        for (int k = 0; k < kLaneTokens; ++k) mine[k] = k < cnt ? tok[first + k] : 0u;
        unsigned nbits = 0;
#pragma unroll
        for (int k = 0; k < kLaneTokens; ++k) {
            unsigned v0, v1;
            int n0, n1;
            token_bits(mine[k], code, v0, n0, v1, n1);
            if (k < cnt) nbits += (unsigned)(n0 + n1);
        }
        unsigned incl = nbits;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned upv = __shfl_up(incl, o);
            if (lane >= o) incl += upv;
        }
        const unsigned pass_bits = carry + __shfl(incl, 63);
        {
            const unsigned pos = carry + incl - nbits;
            unsigned word = pos >> 5;
            int nb = (int)(pos & 31);
            unsigned long long acc = 0;
#pragma unroll
            for (int k = 0; k < kLaneTokens; ++k) {
                if (k >= cnt) break;
                unsigned v[2];
                int n[2];
                token_bits(mine[k], code, v[0], n[0], v[1], n[1]);
#pragma unroll
                for (int piece = 0; piece < 2; ++piece) {           // (31 + 28 bits at most: the accumulator holds a piece)
                    acc |= (unsigned long long)v[piece] << nb;
                    nb += n[piece];
                    if (nb >= 32) {
                        atomicOr(&bits[word], (unsigned)acc);
                        ++word;
                        acc >>= 32;
                        nb -= 32;
                    }
                }
            }
            if (nb > 0 && acc) atomicOr(&bits[word], (unsigned)acc);
        }
        __syncthreads();
        const int nbytes = (int)(pass_bits >> 3);
        flush_bytes(out, out_cap, at, bits, nbytes, lane);
        at += nbytes;
        carry = pass_bits & 7u;
        last = (bits[nbytes >> 2] >> (8 * (nbytes & 3))) & ((1u << carry) - 1u);
        __syncthreads();
        for (unsigned i = lane; i <= (pass_bits >> 5) + 1 && i < (unsigned)kLzBitWords; i += 64) bits[i] = i == 0 ? last : 0u;
        __syncthreads();
    }
    // ---- end-of-block | 000 | pad | 00 00 FF FF
    const unsigned eob = code[256];
    const unsigned end_bits = carry + (eob >> 16) + 3;
    const int end_bytes = (int)((end_bits + 7) >> 3);
    if (lane == 0) {
        const unsigned long long v = (unsigned long long)bits[0] | ((unsigned long long)(eob & 0xffffu) << carry) |
                                     (0xffff0000ull << (8 * end_bytes));
        bits[0] = (unsigned)v;
        bits[1] = (unsigned)(v >> 32);
        bits[2] = 0u;
    }
    __syncthreads();
    flush_bytes(out, out_cap, at, bits, end_bytes + 4, lane);
}

// ---------------------------------------------------------------------------------------------------------------------------
// CRC-32 of every file's IDAT tag + data, in place.  zlib's CRC: reflected, P = 0xEDB88320, a polynomial's x^0 is bit 31.  By
// linearity the register after a message M from the preset I is  raw(M) ^ I x^(8 |M|) mod P,  raw = the register from zero, and
// raw(A | B) = raw(A) x^(8 |B|) ^ raw(B).  Chunks: one thread takes 256 bytes of `out` (cut on the buffer's own grid: a chunk may
// touch several small files), computes raw() of the part inside a file's range by table, multiplies it by x^(8 * bytes behind it)
// and XORs it into the file's accumulator (global atomic; a wave whose lanes all add to one file reduces first) - XOR commutes, so
// the result does not depend on the order.  Store: per file the preset term, the final inversion, four big-endian bytes.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr unsigned kCrcPoly = 0xEDB88320u;
constexpr int kCrcChunk = 256, kCrcThreads = 256;

SDV_DEVICE unsigned gf_mul(unsigned a, unsigned b) {      // a * b mod P
    unsigned p = 0;
#pragma unroll 1
    for (unsigned m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
SDV_DEVICE unsigned gf_x8n(long long nbytes) {            // x^(8 nbytes) mod P
    unsigned p = 1u << 31, sq = 1u << 23;                 // x^0, x^8
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1) p = gf_mul(p, sq);
        sq = gf_mul(sq, sq);
    }
    return p;
}

__global__ __launch_bounds__(kCrcThreads) void png_crc_chunk_kernel(const uint8_t* __restrict__ out, long long out_cap,
                                                                    const long long* __restrict__ offsets, int n,
                                                                    const long long* __restrict__ needed, uint32_t* __restrict__ acc) {
    __shared__ unsigned table[256];
    const long long total = *needed;
    if (total > out_cap) return;
    {
        unsigned c = threadIdx.x;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        table[threadIdx.x] = c;
    }
    __syncthreads();
    const long long c0 = ((long long)blockIdx.x * kCrcThreads + threadIdx.x) * kCrcChunk;
    const long long c1 = min(c0 + kCrcChunk, total);
    int k = n;                                            // the file that holds byte c0 (none: this thread has no bytes)
    if (c0 < total) {
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (offsets[mid] <= c0) lo = mid; else hi = mid - 1;
        }
        k = lo;
    }
    const int k_first = k;
    unsigned mine = 0;
    for (; k < n && offsets[k] < c1; ++k) {
        const long long lo = offsets[k] + 37, hi = offsets[k + 1] - 16;
        const long long a = max(lo, c0), b = min(hi, c1);
        if (a >= b) continue;
        unsigned crc = 0;
        for (long long p = a; p < b; ++p) crc = table[(crc ^ out[p]) & 0xffu] ^ (crc >> 8);
        crc = gf_mul(crc, gf_x8n(hi - b));
        if (k == k_first) mine = crc;
        else atomicXor(&acc[k], crc);
    }
    // (all 64 lanes are here) the first file of every lane: one atomic for the wave where it is the same file for all
    const int k0 = __shfl(k_first, 0);
    const bool same = __all(k_first == k0);
    if (same) {
        unsigned v = mine;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0 && k0 < n && v) atomicXor(&acc[k0], v);
    } else if (k_first < n && mine) {
        atomicXor(&acc[k_first], mine);
    }
}

__global__ __launch_bounds__(64) void png_crc_store_kernel(uint8_t* __restrict__ out, long long out_cap, const long long* __restrict__ offsets,
                                                           int n, const long long* __restrict__ needed, const uint32_t* __restrict__ acc) {
    if (*needed > out_cap) return;
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const long long lo = offsets[k] + 37, hi = offsets[k + 1] - 16;
    if (hi < lo) return;
    const unsigned crc = acc[k] ^ gf_mul(0xffffffffu, gf_x8n(hi - lo)) ^ 0xffffffffu;
#pragma unroll
    for (int b = 0; b < 4; ++b) put_byte(out, out_cap, hi + b, (crc >> (24 - 8 * b)) & 0xffu);
}

// Both packers: the checks, the layout of the two scratch buffers and the launches.  lz: the matching mode.
int deflate_pack(const char* name, bool lz, const uint8_t* filtered, const uint32_t* adler_rows, int32_t n, int32_t H, int32_t W,
                 int32_t stripe_rows, const uint8_t* header, int32_t header_len, void* scratch, int64_t scratch_bytes, void* lz_scratch,
                 int64_t lz_scratch_bytes, uint8_t* out, int64_t out_cap, int64_t* offsets, int64_t* needed, uint8_t* lengths,
                 uint8_t* ll_lengths, uint8_t* d_lengths, void* stream) {
    SDV_REQUIRE(filtered && adler_rows && header && scratch && out && offsets && needed && (!lz || lz_scratch), "%s: null pointer", name);
    SDV_REQUIRE(n > 0 && n <= 65535, "%s: bad frame count n=%d (1 .. 65535)", name, n);
    SDV_REQUIRE(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "%s: bad frame size H=%d W=%d (1 .. 16384)", name, H, W);
    SDV_REQUIRE(stripe_rows >= 1 && stripe_rows <= H, "%s: bad stripe_rows=%d (1 .. H=%d)", name, stripe_rows, H);
    SDV_REQUIRE(header_len == 33, "%s: bad header length %d (signature + IHDR chunk = 33)", name, header_len);
    SDV_REQUIRE(out_cap >= 0, "%s: negative output capacity", name);
    const int stripes = (H + stripe_rows - 1) / stripe_rows;
    const long long n_stripes = (long long)n * stripes;
    SDV_REQUIRE(n_stripes < 0x7fffffffLL, "%s: too many stripes for one grid", name);
    const long long want = 16 * n_stripes + 8 * (((long long)n + 1) / 2) + 4LL * kCodeWords * n_stripes;
    SDV_REQUIRE(scratch_bytes >= want, "%s: scratch buffer too small: %lld bytes, %lld stripes of %d frames need %lld", name,
                (long long)scratch_bytes, n_stripes, n, want);
    SDV_REQUIRE((((uintptr_t)filtered) & 3) == 0 && (((uintptr_t)adler_rows) & 3) == 0 && (((uintptr_t)scratch) & 7) == 0 &&
                    (((uintptr_t)offsets) & 7) == 0 && (((uintptr_t)needed) & 7) == 0,
                "%s: filtered / adler_rows must be 4-byte, scratch / offsets / needed 8-byte aligned", name);
    long long* starts = (long long*)scratch;            // starts [n_stripes] int64 | lens [n_stripes] int64 | Adler-32 [n] | codes
    long long* lens = starts + n_stripes;
    uint32_t* adlers = (uint32_t*)(lens + n_stripes);
    uint32_t* codes = adlers + 2 * (((long long)n + 1) / 2);
    const long long R = 1 + 3LL * W, total_bytes = (long long)n * H * R;
    uint32_t* tokens = (uint32_t*)lz_scratch;           // tokens [n H R] uint32 | token counts [n_stripes, even] | code words [n_stripes][320]
    uint32_t* tok_counts = lz ? tokens + total_bytes : nullptr;
    uint32_t* lz_codes = lz ? tok_counts + 2 * ((n_stripes + 1) / 2) : nullptr;
    if (lz) {
        const long long lz_want = 4 * total_bytes + 8 * ((n_stripes + 1) / 2) + 4LL * kLzCodeWords * n_stripes;
        SDV_REQUIRE(lz_scratch_bytes >= lz_want, "%s: token scratch too small: %lld bytes, %lld filtered bytes in %lld stripes need %lld", name,
                    (long long)lz_scratch_bytes, total_bytes, n_stripes, lz_want);
        SDV_REQUIRE((((uintptr_t)lz_scratch) & 7) == 0, "%s: the token scratch must be 8-byte aligned", name);
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(png_count_kernel, dim3((unsigned)n_stripes), dim3(64), 0, s, filtered, total_bytes, H, R, stripe_rows, stripes, lens, codes,
                       lengths);
    SDV_CHECK_LAUNCH("sdv_png_deflate_pack (count)");
    if (lz) {
        hipLaunchKernelGGL(png_match_kernel, dim3((unsigned)n_stripes), dim3(64), 0, s, filtered, H, R, stripe_rows, stripes, (const uint32_t*)codes,
                           tokens, tok_counts);
        SDV_CHECK_LAUNCH("sdv_png_deflate_lz_pack (match)");
        hipLaunchKernelGGL(png_lz_count_kernel, dim3((unsigned)n_stripes), dim3(64), 0, s, H, R, stripe_rows, stripes, (const uint32_t*)tokens,
                           (const uint32_t*)tok_counts, (const uint32_t*)codes, lz_codes, lens, ll_lengths, d_lengths);
        SDV_CHECK_LAUNCH("sdv_png_deflate_lz_pack (token count)");
    }
    hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, (const long long*)lens, starts, n_stripes, stripes, n, H, R, adler_rows,
                       adlers, (long long*)offsets, (long long*)needed);
    SDV_CHECK_LAUNCH("sdv_png_deflate_pack (scan)");
    hipLaunchKernelGGL(png_write_kernel, dim3((unsigned)n_stripes), dim3(64), 0, s, filtered, total_bytes, H, R, stripe_rows, stripes,
                       (const long long*)starts, (const long long*)lens, (const uint32_t*)codes, (const uint32_t*)adlers, header,
                       (const long long*)offsets, out, (long long)out_cap, (const long long*)needed, (const uint32_t*)tok_counts);
    SDV_CHECK_LAUNCH("sdv_png_deflate_pack (write)");
    if (lz) {
        hipLaunchKernelGGL(png_lz_write_kernel, dim3((unsigned)n_stripes), dim3(64), 0, s, H, R, stripe_rows, stripes, (const uint32_t*)tokens,
                           (const uint32_t*)tok_counts, (const long long*)starts, (const long long*)lens, (const uint32_t*)lz_codes,
                           (const uint32_t*)adlers, header, (const long long*)offsets, out, (long long)out_cap, (const long long*)needed);
        SDV_CHECK_LAUNCH("sdv_png_deflate_lz_pack (token write)");
    }
    return SDV_OK;
}

}  // namespace

extern "C" int sdv_png_deflate_pack(const uint8_t* filtered, const uint32_t* adler_rows, int32_t n, int32_t H, int32_t W, int32_t stripe_rows,
                                    const uint8_t* header, int32_t header_len, void* scratch, int64_t scratch_bytes, uint8_t* out,
                                    int64_t out_cap, int64_t* offsets, int64_t* needed, uint8_t* lengths, void* stream) {
    return deflate_pack("sdv_png_deflate_pack", false, filtered, adler_rows, n, H, W, stripe_rows, header, header_len, scratch, scratch_bytes,
                        nullptr, 0, out, out_cap, offsets, needed, lengths, nullptr, nullptr, stream);
}

extern "C" int sdv_png_deflate_lz_pack(const uint8_t* filtered, const uint32_t* adler_rows, int32_t n, int32_t H, int32_t W,
                                       int32_t stripe_rows, const uint8_t* header, int32_t header_len, void* scratch, int64_t scratch_bytes,
                                       uint8_t* out, int64_t out_cap, int64_t* offsets, int64_t* needed, uint8_t* lengths, void* lz_scratch,
                                       int64_t lz_scratch_bytes, uint8_t* ll_lengths, uint8_t* d_lengths, void* stream) {
    return deflate_pack("sdv_png_deflate_lz_pack", true, filtered, adler_rows, n, H, W, stripe_rows, header, header_len, scratch, scratch_bytes,
                        lz_scratch, lz_scratch_bytes, out, out_cap, offsets, needed, lengths, ll_lengths, d_lengths, stream);
}

extern "C" int sdv_png_crc32(uint8_t* out, int64_t out_cap, const int64_t* offsets, const int64_t* needed, int32_t n, uint32_t* acc,
                             void* stream) {
    SDV_REQUIRE(out && offsets && needed && acc, "sdv_png_crc32: null pointer");
    SDV_REQUIRE(n > 0 && n <= 65535, "sdv_png_crc32: bad frame count n=%d (1 .. 65535)", n);
    SDV_REQUIRE(out_cap >= 0, "sdv_png_crc32: negative output capacity");
    SDV_REQUIRE((((uintptr_t)offsets) & 7) == 0 && (((uintptr_t)needed) & 7) == 0 && (((uintptr_t)acc) & 3) == 0,
                "sdv_png_crc32: offsets / needed must be 8-byte, acc 4-byte aligned");
    const long long chunks = ((long long)out_cap + kCrcChunk - 1) / kCrcChunk;
    const long long blocks = (chunks + kCrcThreads - 1) / kCrcThreads;
    SDV_REQUIRE(blocks < 0x7fffffffLL, "sdv_png_crc32: output capacity too large for one grid");
    if (blocks == 0) return SDV_OK;                     // (nothing fits a buffer of no bytes: *needed > out_cap)
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(acc, 0, 4 * (size_t)n, s) != hipSuccess) {
        sdv_set_error("sdv_png_crc32: clearing the accumulators failed: %s", hipGetErrorString(hipGetLastError()));
        return SDV_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(png_crc_chunk_kernel, dim3((unsigned)blocks), dim3(kCrcThreads), 0, s, (const uint8_t*)out, (long long)out_cap,
                       (const long long*)offsets, n, (const long long*)needed, acc);
    SDV_CHECK_LAUNCH("sdv_png_crc32 (chunks)");
    hipLaunchKernelGGL(png_crc_store_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, out, (long long)out_cap, (const long long*)offsets, n,
                       (const long long*)needed, (const uint32_t*)acc);
    SDV_CHECK_LAUNCH("sdv_png_crc32 (store)");
    return SDV_OK;
}

extern "C" int sdv_png_filter_u8(const uint8_t* frames, int32_t n, int32_t H, int32_t W, uint8_t* filtered, uint32_t* adler_rows,
                                 void* stream) {
    SDV_REQUIRE(frames && filtered && adler_rows, "sdv_png_filter_u8: null pointer");
    SDV_REQUIRE(n > 0 && n <= 65535, "sdv_png_filter_u8: bad frame count n=%d (1 .. 65535)", n);
    SDV_REQUIRE(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "sdv_png_filter_u8: bad frame size H=%d W=%d (1 .. 16384)", H, W);
    SDV_REQUIRE((((uintptr_t)adler_rows) & 3) == 0, "sdv_png_filter_u8: adler_rows must be 4-byte aligned");
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((long long)n * H)), dim3(kFilterThreads), 0, (hipStream_t)stream, frames, filtered,
                       adler_rows, H, W);
    SDV_CHECK_LAUNCH("sdv_png_filter_u8");
    return SDV_OK;
}

