// Baseline JPEG encoding of drawn frames: u8 frames resident on the device -> the entropy-coded data of every
// frame in one packed payload, so that only compressed bytes cross to the host.  Contract and THE RULE: include/gomatching_hip.h;
// the statement the kernels are held to byte for byte: tests/jpeg_statement.py; the numpy twin: gomatching_amd/jpeg.py.
// Integers only, no atomics, no scratch, every output word has one writer, nothing depends on launch order.
//
// Four launches over one workspace in HBM (gom_jpeg_workspace_bytes):
//   jpeg_transform_kernel  a wavefront per MCU (four MCUs per 256-thread workgroup).  Lane l loads pixels l, l + 64, .. of the
//                          16 x 16 (coordinates clamped: the replicated last column and row), converts them and leaves the
//                          level-shifted luminance blocks and the full-resolution chrominance in LDS; lane (y, x) takes the
//                          2 x 2 means; then the two passes of the DCT, a lane per output ((y, u), then (v, u)) with its row of
//                          the table in eight registers, through LDS between them; the lane quantises its coefficient and stores
//                          it at its zigzag position: int16 [block][64], blocks in coding order.
//   jpeg_entropy_kernel    a workgroup per restart interval (one MCU row of one frame).  A lane per block walks its 64
//                          coefficients (eight 16-byte loads), forms the code words in a 64-bit accumulator and stages them,
//                          most significant bit first, in the block's own 52 words of HBM (a block's code is at most 1 660
//                          bits); the bit lengths go to LDS and are scanned (thread-serial chunks around a shuffle scan).  Then
//                          every lane OWNS a 32-bit word of the interval's bit stream: it finds the block that holds the word's
//                          first bit by binary search in the scanned starts and gathers the word from the staged blocks (the
//                          bits behind the last block are the 1-padding).  The word stays in registers: a second scan, over
//                          the words' counts of 0xFF bytes, gives the lane the place of its four bytes behind the stuffed zeros
//                          of all earlier words, and it writes them (and a zero behind each 0xFF) into the interval's stuffed
//                          staging; thread 0 appends RSTn and stores the length.  Staging lives in HBM, not LDS: 480 blocks of
//                          a 1280-wide row would fit (98 KiB), 1 536 blocks of a 4096-wide one would not (312 KiB).
//   jpeg_offsets_kernel    one workgroup: the exclusive scan of the interval lengths (int64) and, from it, the F + 1 frame offsets.
//   jpeg_pack_kernel       a thread OWNS a 32-bit word of the payload: binary search for the interval of its first byte, then
//                          up to four bytes gathered from one or more intervals' stuffed staging.
// The width limit GOM_JPEG_MAX_WIDTH = 4096 is the size of the LDS array of block starts (1 537 ints).
#include "common.h"
#include "wave_block.h"

#define JP_THREADS 256
#define JP_STAGE_WORDS 52                                              // 1 660 bits of a block's code, rounded up to words
#define JP_MAX_NB (6 * (GOM_JPEG_MAX_WIDTH / 16))                      // blocks of a restart interval

namespace {

// ---- tables ---------------------------------------------------------------------------------------------------------------
__constant__ short jp_T[64] = {2896, 2896,  2896,  2896,  2896,  2896,  2896,  2896,  4017, 3406,  2276,  799,   -799,  -2276, -3406, -4017,
                               3784, 1567,  -1567, -3784, -3784, -1567, 1567,  3784,  3406, -799,  -4017, -2276, 2276,  4017,  799,   -3406,
                               2896, -2896, -2896, 2896,  2896,  -2896, -2896, 2896,  2276, -4017, 799,   3406,  -3406, -799,  4017,  -2276,
                               1567, -3784, 3784,  -1567, -1567, 3784,  -3784, 1567,  799,  -2276, 3406,  -4017, 4017,  -3406, 2276,  -799};
// zigzag position of the coefficient with natural index v * 8 + u
__constant__ unsigned char jp_zzpos[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                           41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                           46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
__constant__ unsigned char jp_qbase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26,  58,  60,  55, 14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3 - K.6: BITS and HUFFVAL; the code tables are made from them at compile time (Annex C)
constexpr unsigned char JP_DC_LUM_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr unsigned char JP_DC_CHR_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr unsigned char JP_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char JP_AC_LUM_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr unsigned char JP_AC_LUM_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr unsigned char JP_AC_CHR_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr unsigned char JP_AC_CHR_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// entry = length << 16 | code; [0] luminance, [1] chrominance
struct JpTabs {
    unsigned dc[2][12];
    unsigned ac[2][256];
};
constexpr void jp_fill(unsigned* tab, const unsigned char* bits, const unsigned char* vals) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) tab[vals[k++]] = ((unsigned)len << 16) | code++;
        code <<= 1;
    }
}
constexpr JpTabs jp_make_tabs() {
    JpTabs t{};
    jp_fill(t.dc[0], JP_DC_LUM_BITS, JP_DC_VALS);
    jp_fill(t.dc[1], JP_DC_CHR_BITS, JP_DC_VALS);
    jp_fill(t.ac[0], JP_AC_LUM_BITS, JP_AC_LUM_VALS);
    jp_fill(t.ac[1], JP_AC_CHR_BITS, JP_AC_CHR_VALS);
    return t;
}
__constant__ JpTabs jp_tabs = jp_make_tabs();

// ---- the workspace ----------------------------------------------------------------------------------------------------------
struct JpLayout {
    int MH, MW, nb;                                                    // MCU rows, MCUs per row, blocks per interval
    long NI, n_mcu, n_blk;                                             // intervals, MCUs, blocks of the call
    long cap;                                                          // bytes of an interval's stuffed staging
    long coef, stage, stuffed, lens, ioff, total;                      // byte offsets, 256-aligned, and the size
};

inline long jp_align(long v) { return (v + 255) / 256 * 256; }

// false: the sizes do not fit the kernels' index types
inline bool jp_layout(int F, int H, int W, JpLayout& L) {
    L.MH = (H + 15) / 16;
    L.MW = (W + 15) / 16;
    L.nb = 6 * L.MW;
    L.NI = (long)F * L.MH;
    L.n_mcu = L.NI * L.MW;
    L.n_blk = L.n_mcu * 6;
    L.cap = (long)L.nb * (2 * JP_STAGE_WORDS * 4) + 16;                // every byte 0xFF, and the marker
    if (L.NI > 2147483647L || L.n_mcu > 2147483647L) return false;
    L.coef = 0;
    L.stage = jp_align(L.coef + L.n_blk * 128);
    L.stuffed = jp_align(L.stage + L.n_blk * (JP_STAGE_WORDS * 4));
    L.lens = jp_align(L.stuffed + L.NI * L.cap);
    L.ioff = jp_align(L.lens + L.NI * 4);
    L.total = jp_align(L.ioff + (L.NI + 1) * 8);
    return true;
}

// (the exclusive scans of one int per thread over the workgroup: wb_block_excl_scan of wave_block.h, two barriers each)

// ---- launch 1: colour, 2x2 mean, DCT, quantisation, zigzag --------------------------------------------------------------------
__global__ __launch_bounds__(JP_THREADS) void jpeg_transform_kernel(const unsigned char* __restrict__ frames, int H, int W, int MH,
                                                                    int MW, long n_mcu, int bgr, int scale, short* __restrict__ coef) {
    __shared__ short s_blk[JP_THREADS / 64][6][64];
    __shared__ short s_c[JP_THREADS / 64][2][256];
    __shared__ int s_tmp[JP_THREADS / 64][6][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long m = (long)blockIdx.x * (JP_THREADS / 64) + wave;
    const bool live = m < n_mcu;
    const long mc = live ? m : n_mcu - 1;                              // a spare wave repeats the last MCU and stores nothing
    const int mx = (int)(mc % MW);
    const long row = mc / MW;
    const int my = (int)(row % MH);
    const unsigned char* base = frames + (size_t)(row / MH) * H * W * 3;

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = lane + 64 * i, y = p >> 4, x = p & 15;
        const int sy = min(16 * my + y, H - 1), sx = min(16 * mx + x, W - 1);
        const unsigned char* px = base + ((size_t)sy * W + sx) * 3;
        const int c0 = px[0], g = px[1], c2 = px[2];
        const int r = bgr ? c2 : c0, b = bgr ? c0 : c2;
        const int Y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
        const int cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
        const int cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
        s_blk[wave][(y >> 3) * 2 + (x >> 3)][(y & 7) * 8 + (x & 7)] = (short)(Y - 128);
        s_c[wave][0][p] = (short)cb;
        s_c[wave][1][p] = (short)cr;
    }
    __syncthreads();
    {
        const int o = (lane >> 3) * 32 + (lane & 7) * 2;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            s_blk[wave][4 + c][lane] = (short)(((s_c[wave][c][o] + s_c[wave][c][o + 1] + s_c[wave][c][o + 16] + s_c[wave][c][o + 17] + 2) >> 2) - 128);
    }
    __syncthreads();

    const int u = lane & 7, v = lane >> 3;                             // pass 1: lane = (row y = v, frequency u); pass 2: (v, u)
    int tu[8], tv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        tu[k] = jp_T[u * 8 + k];
        tv[k] = jp_T[v * 8 + k];
    }
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        int acc = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += tu[x] * s_blk[wave][b][v * 8 + x];
        s_tmp[wave][b][lane] = (acc + 128) >> 8;
    }
    __syncthreads();
    const int zz = jp_zzpos[lane];
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        int acc = 0;
#pragma unroll
        for (int y = 0; y < 8; ++y) acc += tv[y] * s_tmp[wave][b][y * 8 + u];
        const int f = (acc + (1 << 17)) >> 18;
        const int q = min(max(((int)jp_qbase[b < 4 ? 0 : 1][lane] * scale + 50) / 100, 1), 255);
        int k = (abs(f) + (q >> 1)) / q;
        if (lane > 0) k = min(k, 1023);
        if (live) coef[(m * 6 + b) * 64 + zz] = (short)(f < 0 ? -k : k);
    }
}

// ---- launch 2: Huffman coding, bit packing, byte stuffing: a workgroup per restart interval ------------------------------------
struct JpBits {
    unsigned long long acc;
    int n, total, wi;
    unsigned* dst;
    __device__ __forceinline__ void put(unsigned v, int len) {         // len <= 26, n < 32 on entry
        acc = (acc << len) | v;
        n += len;
        total += len;
        if (n >= 32) {
            if (wi < JP_STAGE_WORDS) dst[wi] = (unsigned)(acc >> (n - 32));
            ++wi;
            n -= 32;
        }
    }
};

__device__ __forceinline__ void jp_put_value(JpBits& w, unsigned entry, int cat, int value) {
    const unsigned amp = (unsigned)(value < 0 ? value - 1 : value) & ((1u << cat) - 1u);
    w.put(((entry & 0xFFFFu) << cat) | amp, (int)(entry >> 16) + cat);
}

__global__ __launch_bounds__(JP_THREADS) void jpeg_entropy_kernel(const short* __restrict__ coef, int MH, int MW,
                                                                  unsigned* __restrict__ stage, unsigned char* __restrict__ stuffed,
                                                                  long cap, int* __restrict__ lens) {
    __shared__ int s_start[JP_MAX_NB + 1];
    __shared__ int s_red[JP_THREADS / 64];
    const int tid = threadIdx.x;
    const long iv = blockIdx.x;
    const int my = (int)(iv % MH);
    const int nb = 6 * MW;                                             // <= JP_MAX_NB: the host refuses wider images
    const short* c0 = coef + iv * nb * 64;
    unsigned* st0 = stage + iv * nb * JP_STAGE_WORDS;

    // A: a lane per block
    for (int j = tid; j < nb; j += JP_THREADS) {
        const int k = j % 6, m = j / 6;
        const int prev = k == 0 ? (m > 0 ? j - 3 : -1) : (k < 4 ? j - 1 : (m > 0 ? j - 6 : -1));
        const int pred = prev >= 0 ? (int)c0[(long)prev * 64] : 0;
        const int ch = k < 4 ? 0 : 1;
        const uint4* src = reinterpret_cast<const uint4*>(c0 + (long)j * 64);
        JpBits w = {0ull, 0, 0, 0, st0 + (long)j * JP_STAGE_WORDS};
        int run = 0;
        for (int q = 0; q < 8; ++q) {
            const uint4 v4 = src[q];
            const unsigned wd[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = (int)(short)(wd[e >> 1] >> ((e & 1) * 16));
                if (q == 0 && e == 0) {
                    const int d = c - pred;
                    const int cat = min(32 - __clz(abs(d)), 11);
                    jp_put_value(w, jp_tabs.dc[ch][cat], cat, d);
                } else if (c == 0) {
                    ++run;
                } else {
                    while (run > 15) {
                        w.put(jp_tabs.ac[ch][0xF0] & 0xFFFFu, (int)(jp_tabs.ac[ch][0xF0] >> 16));
                        run -= 16;
                    }
                    const int cat = min(32 - __clz(abs(c)), 10);
                    jp_put_value(w, jp_tabs.ac[ch][(run << 4) | cat], cat, c);
                    run = 0;
                }
            }
        }
        if (run > 0) w.put(jp_tabs.ac[ch][0] & 0xFFFFu, (int)(jp_tabs.ac[ch][0] >> 16));
        if (w.n > 0 && w.wi < JP_STAGE_WORDS) w.dst[w.wi] = (unsigned)(w.acc << (32 - w.n));
        s_start[j] = w.total;
    }
    __syncthreads();

    // B: lengths -> starts, s_start[nb] = the interval's bits
    {
        const int chunk = (nb + JP_THREADS - 1) / JP_THREADS;
        const int a = min(tid * chunk, nb), b = min(a + chunk, nb);
        int sum = 0;
        for (int j = a; j < b; ++j) sum += s_start[j];
        int total;
        int at = wb_block_excl_scan<JP_THREADS>(sum, s_red, total);
        for (int j = a; j < b; ++j) {
            const int len = s_start[j];
            s_start[j] = at;
            at += len;
        }
        if (tid == 0) s_start[nb] = total;
    }
    __syncthreads();

    // C, D: a lane per word of the bit stream, 256 words a round
    const int T = s_start[nb];
    const int nbytes = (T + 7) >> 3, nwords = (nbytes + 3) >> 2;
    unsigned char* out = stuffed + iv * cap;
    int carry = 0;
    for (int base = 0; base < nwords; base += JP_THREADS) {
        const int wi = base + tid;
        unsigned word = 0;
        int nv = 0;
        if (wi < nwords) {
            nv = min(4, nbytes - 4 * wi);
            int pos = 32 * wi;
            int lo = 0, hi = nb + 1;                                   // the first start above pos; s_start[0] = 0 <= pos
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_start[mid] <= pos) lo = mid + 1;
                else hi = mid;
            }
            int j = lo - 1, got = 0;
            while (got < 32) {
                if (j >= nb) {                                         // behind the last block: the padding
                    word |= 0xFFFFFFFFu >> got;
                    break;
                }
                const int s0 = s_start[j], s1 = s_start[j + 1];
                const int off = pos - s0, avail = s1 - pos;
                if (avail <= 0 || off < 0 || off >= JP_STAGE_WORDS * 32) {
                    ++j;
                    continue;
                }
                const int take = min(32 - got, avail);
                const unsigned* st = st0 + (long)j * JP_STAGE_WORDS;
                const int sw = off >> 5, sh = off & 31;
                const unsigned long long two = ((unsigned long long)st[sw] << 32) | (sw + 1 < JP_STAGE_WORDS ? st[sw + 1] : 0u);
                const unsigned bits = (unsigned)((two << sh) >> (64 - take));
                word |= bits << (32 - got - take);
                got += take;
                pos += take;
            }
        }
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) cnt += (i < nv && ((word >> (24 - 8 * i)) & 255u) == 255u) ? 1 : 0;
        int tot;
        const int excl = wb_block_excl_scan<JP_THREADS>(cnt, s_red, tot);
        if (nv > 0) {
            long p = 4L * wi + carry + excl;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned b = (word >> (24 - 8 * i)) & 255u;
                if (i < nv && p + 1 < cap) {
                    out[p++] = (unsigned char)b;
                    if (b == 255u) out[p++] = 0;
                }
            }
        }
        carry += tot;
    }
    if (tid == 0) {
        int len = nbytes + carry;
        if (my + 1 < MH && len + 2 <= cap) {
            out[len] = 0xFF;
            out[len + 1] = (unsigned char)(0xD0 + (my & 7));
            len += 2;
        }
        lens[iv] = len;
    }
}

// ---- launch 3: interval lengths -> interval and frame offsets ---------------------------------------------------------------------
__global__ __launch_bounds__(JP_THREADS) void jpeg_offsets_kernel(const int* __restrict__ lens, long NI, int MH, int F, long cap,
                                                                  long long* __restrict__ ioff, long long* __restrict__ frame_off) {
    __shared__ int s_red[JP_THREADS / 64];
    const int tid = threadIdx.x;
    long long carry = 0;
    for (long base = 0; base < NI; base += JP_THREADS) {
        const long i = base + tid;
        const int v = i < NI ? min(max(lens[i], 0), (int)min(cap, 8388607L)) : 0;   // 256 of them fit an int
        int tot;
        const int excl = wb_block_excl_scan<JP_THREADS>(v, s_red, tot);
        if (i < NI) {
            ioff[i] = carry + excl;
            if (i % MH == 0) frame_off[i / MH] = carry + excl;
        }
        carry += tot;
    }
    if (tid == 0) {
        ioff[NI] = carry;
        frame_off[F] = carry;
    }
}

// ---- launch 4: the packed payload, a thread per word ---------------------------------------------------------------------------
__global__ __launch_bounds__(JP_THREADS) void jpeg_pack_kernel(const unsigned char* __restrict__ stuffed, long cap,
                                                               const long long* __restrict__ ioff, long NI, long total,
                                                               unsigned* __restrict__ payload, long nwords) {
    const long k = (long)blockIdx.x * JP_THREADS + threadIdx.x;
    if (k >= nwords) return;
    const long long p0 = 4 * k;
    long lo = 0, hi = NI + 1;                                          // the first offset above p0; ioff[0] = 0 <= p0
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (ioff[mid] <= p0) lo = mid + 1;
        else hi = mid;
    }
    long i = lo - 1;
    unsigned word = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const long long p = p0 + b;
        unsigned byte = 0;
        if (p < total) {
            while (i < NI && p >= ioff[i + 1]) ++i;
            if (i < NI) {
                const long long off = p - ioff[i];
                if (off >= 0 && off < cap) byte = stuffed[i * cap + off];
            }
        }
        word |= byte << (8 * b);
    }
    payload[k] = word;
}

int jp_check(const void* frames_or_ws, int F, int H, int W) {
    if (!frames_or_ws || F < 0 || H < 1 || W < 1) return GOM_ERR_INVALID_ARG;
    if (W > GOM_JPEG_MAX_WIDTH || H > GOM_JPEG_MAX_HEIGHT) return GOM_ERR_UNSUPPORTED;
    return GOM_OK;
}

}  // namespace

extern "C" long gom_jpeg_workspace_bytes(int F, int H, int W) {
    JpLayout L;
    if (F < 0 || H < 1 || W < 1 || W > GOM_JPEG_MAX_WIDTH || H > GOM_JPEG_MAX_HEIGHT || !jp_layout(F, H, W, L)) return -1;
    return L.total;
}

extern "C" int gom_jpeg_encode_scan_u8(const uint8_t* frames, int F, int H, int W, int bgr, int quality, void* workspace,
                                       long workspace_bytes, int64_t* frame_off, void* stream) {
    GOM_CHECK_ARG(quality >= 1 && quality <= 100 && (bgr == 0 || bgr == 1) && workspace && frame_off);
    const int rc = jp_check(frames, F, H, W);
    if (rc != GOM_OK) return rc;
    JpLayout L;
    if (!jp_layout(F, H, W, L)) return GOM_ERR_UNSUPPORTED;
    GOM_CHECK_ARG(workspace_bytes >= L.total && ((uintptr_t)workspace & 255) == 0);
    if (F == 0) return GOM_OK;
    unsigned char* ws = (unsigned char*)workspace;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)((L.n_mcu + 3) / 4)), dim3(JP_THREADS), 0, (hipStream_t)stream,
                       (const unsigned char*)frames, H, W, L.MH, L.MW, L.n_mcu, bgr, scale, (short*)(ws + L.coef));
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)L.NI), dim3(JP_THREADS), 0, (hipStream_t)stream,
                       (const short*)(ws + L.coef), L.MH, L.MW, (unsigned*)(ws + L.stage), ws + L.stuffed, L.cap, (int*)(ws + L.lens));
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(JP_THREADS), 0, (hipStream_t)stream, (const int*)(ws + L.lens), L.NI, L.MH,
                       F, L.cap, (long long*)(ws + L.ioff), (long long*)frame_off);
    return gom_launch_status();
}

extern "C" int gom_jpeg_encode_pack_u8(const void* workspace, long workspace_bytes, int F, int H, int W, long total,
                                       uint8_t* payload, long payload_bytes, void* stream) {
    GOM_CHECK_ARG(total >= 0 && payload_bytes >= 0);
    const int rc = jp_check(workspace, F, H, W);
    if (rc != GOM_OK) return rc;
    JpLayout L;
    if (!jp_layout(F, H, W, L)) return GOM_ERR_UNSUPPORTED;
    const long nwords = (total + 3) / 4;
    GOM_CHECK_ARG(workspace_bytes >= L.total && ((uintptr_t)workspace & 255) == 0);
    GOM_CHECK_ARG(total <= L.NI * L.cap && payload_bytes >= 4 * nwords && nwords <= 2147483647L * JP_THREADS);
    if (nwords == 0) return GOM_OK;
    GOM_CHECK_ARG(payload && ((uintptr_t)payload & 3) == 0);
    const unsigned char* ws = (const unsigned char*)workspace;
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)((nwords + JP_THREADS - 1) / JP_THREADS)), dim3(JP_THREADS), 0,
                       (hipStream_t)stream, ws + L.stuffed, L.cap, (const long long*)(ws + L.ioff), L.NI, total, (unsigned*)payload,
                       nwords);
    return gom_launch_status();
}
