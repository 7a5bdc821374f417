// Training augmentation of the replay-pool input (include/adaisp.h): adaisp_augment_u8 and adaisp_mosaic_u8 are ONE pass
// with two tap rules. Decoded uint8 HWC BGR sources anywhere in `src` -> one uint8 HWC BGR S x S frame per image: an affine
// warp (random_perspective with perspective = 0, augmentations.py:144-193, and the two flips of dataset.py:505-514 folded
// into the map), then the HSV tables of augment_hsv (augmentations.py:67-80). It runs BEFORE adaisp_unprocess /
// adaisp_unprocess_bayer: the sensor model sees the warped 8-bit scene, so its noise stays white. Everything is integer
// arithmetic; two numpy int64 restatements (tests/_augref.py, tests/_mosaicref.py) match it bit for bit.
//
// Warp, for output pixel (x, y) and an inverse map m[0..5] (Q16, int64; sums wrap modulo 2^64):
//     fx = m0 * x + m1 * y + m2            fy = m3 * x + m4 * y + m5
//     X = fx >> 16, Y = fy >> 16           (arithmetic shift: floor)
//     ax = (fx >> 11) & 31, ay = (fy >> 11) & 31                               (weights in 1/32 pixel)
//     v = ((32 - ax) (32 - ay) P(X, Y) + ax (32 - ay) P(X + 1, Y) + (32 - ax) ay P(X, Y + 1) + ax ay P(X + 1, Y + 1)
//          + 512) >> 10                                                        per channel
// with P(i, j) the kernel's tap rule, each of the four taps on its own, nothing clamped. Coordinates are pixel indices without
// a half-pixel shift (cv2.warpAffine's convention). With the identity map (m = 65536, 0, 0, 0, 65536, 0) v = P(x, y).
//
// Tap rule of adaisp_augment_u8: an image is one source (src_offset, h, w) letterboxed at (top, left) of the S x S frame,
// one map and the launch's `fill`:
//     P(i, j) = the source pixel at row j - top, column i - left when that lies in [0, h) x [0, w), else `fill`
// so the identity map gives the letterboxed frame, byte for byte. A placement that does not fit the frame, or pixels that
// do not lie inside src_bytes, are never read: all fill.
//
// Tap rule of adaisp_mosaic_u8: the same over a canvas made of several sources (load_mosaic, dataloaders.py:758-814) and
// the blend of two such canvases (mixup, augmentations.py:289-294). An image has 1 or 2 layers; a layer is a map m[0..5], a
// `fill` and up to 4 tiles; a tile is a source (src_offset, h, w), a half-open canvas rectangle [x0, x1) x [y0, y1) and
// (dx, dy). fx, fy, X, Y, ax, ay and v are the layer's, with
//     P(i, j) = the pixel at row j - dy, column i - dx of the first tile (in index order) with x0 <= i < x1 and
//               y0 <= j < y1, else the layer's fill
// so taps that straddle a seam between two tiles, or a tile and the fill, blend the two. A tile is absent (never matched,
// never read) when h or w is outside [0, 32768], its rectangle is reversed or maps outside its own source (x0 - dx < 0,
// x1 - dx > w, y0 - dy < 0, y1 - dy > h), or its h * w * 3 bytes do not lie inside src_bytes. n_tiles is taken into [0, 4]
// and mix into [0, 65536]. With two layers (n_layers = 2 in the record AND in the launch) of values v0 and v1, mix in Q16:
//     v = (mix * v0 + (65536 - mix) * v1) >> 16        per channel (rounds down, as .astype(np.uint8) does)
// else v = v0. One layer of one tile at [left, left + w) x [top, top + h) with (dx, dy) = (left, top) is
// adaisp_augment_u8's image, byte for byte. The record (448 bytes) is uniform over a workgroup: it is read through uniform
// (scalar) loads, the tile scan is unrolled and ends in ONE gather per tap, and the second layer's 16 gathers are skipped
// when the image has one layer. adaisp_augment_u8 keeps its own rule and launch: as a one-tile mosaic it is slower.
//
// Colour, when the image has a table (0 <= lut < n_luts), on the warped 8-bit (b, g, r); every `/` is a division of
// non-negative integers rounded down, so (2 n + d) / (2 d) is n / d rounded to nearest, halves up:
//   BGR -> HSV (cv2.COLOR_BGR2HSV's 8-bit ranges: H in [0, 180), S and V in [0, 255]):
//     V = max(b, g, r), d = V - min(b, g, r)
//     S = 0 when V = 0, else (255 d + V / 2) / V
//     H = 0 when d = 0; else with
//         n = 30 (g - b), plus 180 d when that is negative      when V = r
//         n = 30 (b - r) + 60 d                                 else when V = g
//         n = 30 (r - g) + 120 d                                else
//     H = (2 n + d) / (2 d), and 180 becomes 0
//   tables: H' = T[H], S' = T[256 + S], V' = T[512 + V] (768 bytes per image), then H' = H' mod 180
//   HSV -> BGR: i = H' / 30, f = H' - 30 i,
//     p = (V' (255 - S') + 127) / 255
//     q = (V' (7650 - S' f) + 3825) / 7650
//     t = (V' (7650 - S' (30 - f)) + 3825) / 7650
//     (r, g, b) = (V', t, p), (q, V', p), (p, V', t), (p, q, V'), (t, p, V'), (V', p, q)   for i = 0 .. 5
//
// Mapping from the output side (warp_quads, the body both kernels share): a lane owns 4 consecutive pixels of one output
// row (12 bytes: three dword stores when S % 4 == 0 and `dst` is 4-byte aligned, byte stores otherwise) and gathers its
// source pixels with byte loads, so a source may start at any byte offset of `src`; a batch's sources are a few MB and stay
// in the L2. The image's table is copied into LDS once per workgroup (768 bytes, the only LDS).
#include "isp_internal.h"

static_assert(sizeof(adaisp_augment_desc) == 80, "adaisp_augment_desc is 80 bytes (adaptiveisp_amd/_lib.py)");
static_assert(sizeof(adaisp_mosaic_tile) == 40 && sizeof(adaisp_mosaic_layer) == 216 && sizeof(adaisp_mosaic_desc) == 448,
              "adaisp_mosaic_desc is 448 bytes: 2 layers of 216 (4 tiles of 40) (adaptiveisp_amd/_lib.py)");

namespace adaisp {
namespace {

constexpr int AUG_THREADS = 256;

struct Bgr {
    unsigned b, g, r;
};

__device__ __forceinline__ unsigned umin3(unsigned a, unsigned b, unsigned c) { return min(a, min(b, c)); }
__device__ __forceinline__ unsigned umax3(unsigned a, unsigned b, unsigned c) { return max(a, max(b, c)); }

// the header comment's BGR -> HSV -> tables -> BGR
__device__ __forceinline__ Bgr hsv_tables(Bgr c, const uint8_t* lut) {
    const unsigned V = umax3(c.b, c.g, c.r), d = V - umin3(c.b, c.g, c.r);
    const unsigned S = V ? (255u * d + (V >> 1)) / V : 0u;
    unsigned H = 0;
    if (d) {
        int n;
        if (V == c.r) {
            n = 30 * ((int)c.g - (int)c.b);
            if (n < 0) n += 180 * (int)d;
        } else if (V == c.g) {
            n = 30 * ((int)c.b - (int)c.r) + 60 * (int)d;
        } else {
            n = 30 * ((int)c.r - (int)c.g) + 120 * (int)d;
        }
        H = (2u * (unsigned)n + d) / (2u * d);
        if (H >= 180u) H -= 180u;
    }
    const unsigned h = lut[H] % 180u, s = lut[256 + S], v = lut[512 + V];
    const unsigned i = h / 30u, f = h - 30u * i;
    const unsigned p = (v * (255u - s) + 127u) / 255u;
    const unsigned q = (v * (7650u - s * f) + 3825u) / 7650u;
    const unsigned t = (v * (7650u - s * (30u - f)) + 3825u) / 7650u;
    Bgr o;
    o.r = (i == 0 || i == 5) ? v : (i == 1) ? q : (i == 4) ? t : p;
    o.g = (i == 1 || i == 2) ? v : (i == 0) ? t : (i == 3) ? q : p;
    o.b = (i == 3 || i == 4) ? v : (i == 2) ? t : (i == 5) ? q : p;
    return o;
}

// the image's 768-byte table into LDS, by the whole workgroup (AUG_THREADS threads)
__device__ __forceinline__ void load_table(uint8_t* lut, const uint8_t* __restrict__ t) {
#pragma unroll
    for (int k = 0; k < 3; ++k) lut[k * AUG_THREADS + threadIdx.x] = t[k * AUG_THREADS + threadIdx.x];
    __syncthreads();
}

__device__ __forceinline__ Bgr unpack_fill(unsigned fill) { return Bgr{fill & 255u, (fill >> 8) & 255u, (fill >> 16) & 255u}; }

// the header comment's v for the Q16 position (fx, fy): P(i, j) resolves one tap
template <class Tap>
__device__ __forceinline__ Bgr tap_blend(uint64_t fx, uint64_t fy, Tap P) {
    const int64_t X = (int64_t)fx >> 16, Y = (int64_t)fy >> 16;
    const unsigned ax = (unsigned)((int64_t)fx >> 11) & 31u, ay = (unsigned)((int64_t)fy >> 11) & 31u;
    const Bgr p00 = P(X, Y), p10 = P(X + 1, Y), p01 = P(X, Y + 1), p11 = P(X + 1, Y + 1);
    const unsigned w00 = (32u - ax) * (32u - ay), w10 = ax * (32u - ay), w01 = (32u - ax) * ay, w11 = ax * ay;
    Bgr v;
    v.b = (w00 * p00.b + w10 * p10.b + w01 * p01.b + w11 * p11.b + 512u) >> 10;
    v.g = (w00 * p00.g + w10 * p10.g + w01 * p01.g + w11 * p11.g + 512u) >> 10;
    v.r = (w00 * p00.r + w10 * p10.r + w01 * p01.r + w11 * p11.r + 512u) >> 10;
    return v;
}

// a lane's 4 pixels (12 bytes) to row `out`: three dword stores, or byte stores of the pixels left of S
template <bool VEC>
__device__ __forceinline__ void store_quad(uint8_t* __restrict__ out, const uint8_t (&o)[12], int x0, int S) {
    if (VEC) {
        uint32_t* __restrict__ out4 = reinterpret_cast<uint32_t*>(out);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            out4[k] = (uint32_t)o[4 * k] | ((uint32_t)o[4 * k + 1] << 8) | ((uint32_t)o[4 * k + 2] << 16) |
                      ((uint32_t)o[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (x0 + k < S) {
                out[3 * k] = o[3 * k];
                out[3 * k + 1] = o[3 * k + 1];
                out[3 * k + 2] = o[3 * k + 2];
            }
        }
    }
}

// the Q16 position (fx, fy) of a map at the lane's first pixel (x0, y); unsigned: the wrap modulo 2^64 is defined, and numpy's
struct Q16Pos {
    uint64_t fx = 0, fy = 0, sx = 0, sy = 0;
    Q16Pos() = default;
    __device__ __forceinline__ Q16Pos(const int64_t (&m)[6], int x0, int y)
        : fx((uint64_t)m[0] * (uint64_t)x0 + (uint64_t)m[1] * (uint64_t)y + (uint64_t)m[2]),
          fy((uint64_t)m[3] * (uint64_t)x0 + (uint64_t)m[4] * (uint64_t)y + (uint64_t)m[5]),
          sx((uint64_t)m[0]), sy((uint64_t)m[3]) {}
    __device__ __forceinline__ void step() { fx += sx, fy += sy; }
};

// The pass both kernels are: image blockIdx.y's table (`lut_index`; none when outside `luts`) into LDS, the lane's quad,
// its 4 values through the table, one store. `rule(x0, y)` is the kernel's tap rule: it yields the lane's value source,
// a callable that returns the value of the next pixel to the right at every call.
template <bool VEC, class Rule>
__device__ __forceinline__ void warp_quads(int lut_index, const uint8_t* __restrict__ luts, int n_luts,
                                           uint8_t* __restrict__ dst, int S, int quads_per_row, Rule rule) {
    __shared__ uint8_t lut[768];
    const bool colour = lut_index >= 0 && lut_index < n_luts;        // uniform over the workgroup
    if (colour) load_table(lut, luts + (int64_t)lut_index * 768);
    const long q = (long)blockIdx.x * AUG_THREADS + threadIdx.x;
    if (q >= (long)S * quads_per_row) return;
    const int y = (int)(q / quads_per_row), x0 = (int)(q - (long)y * quads_per_row) * 4;
    auto value = rule(x0, y);
    uint8_t o[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        Bgr v = value();
        if (colour) v = hsv_tables(v, lut);
        o[3 * k] = (uint8_t)v.b;
        o[3 * k + 1] = (uint8_t)v.g;
        o[3 * k + 2] = (uint8_t)v.r;
    }
    store_quad<VEC>(dst + ((long)blockIdx.y * S * S + (long)y * S + x0) * 3, o, x0, S);
}

template <bool VEC>
__global__ __launch_bounds__(AUG_THREADS) void k_augment_u8(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                            const adaisp_augment_desc* __restrict__ desc,
                                                            const uint8_t* __restrict__ luts, int n_luts,
                                                            uint8_t* __restrict__ dst, int S, int quads_per_row,
                                                            unsigned fill) {
    const adaisp_augment_desc& d = desc[blockIdx.y];
    warp_quads<VEC>(d.lut, luts, n_luts, dst, S, quads_per_row, [&](int x0, int y) {
        const int h = d.h, w = d.w, top = d.top, left = d.left;
        const bool fits = h >= 0 && w >= 0 && top >= 0 && left >= 0 && top <= S - h && left <= S - w && d.src_offset >= 0 &&
                          d.src_offset <= src_bytes - (int64_t)h * w * 3;
        const uint8_t* __restrict__ img = src + (fits ? d.src_offset : 0);
        const Bgr pad = unpack_fill(fill);
        auto tap = [=](int64_t i, int64_t j) {
            const int64_t ix = i - left, iy = j - top;
            if (!fits || ix < 0 || ix >= w || iy < 0 || iy >= h) return pad;
            const uint8_t* __restrict__ px = img + (iy * w + ix) * 3;
            return Bgr{px[0], px[1], px[2]};
        };
        return [tap, p = Q16Pos(d.m, x0, y)]() mutable {
            const Bgr v = tap_blend(p.fx, p.fy, tap);
            p.step();
            return v;
        };
    });
}

// is the tile there at all (the header comment's rule)? Uniform over the workgroup.
__device__ __forceinline__ bool tile_present(const adaisp_mosaic_tile& t, int64_t src_bytes) {
    const int64_t h = t.h, w = t.w;
    return h >= 0 && w >= 0 && h <= 32768 && w <= 32768 && t.x0 <= t.x1 && t.y0 <= t.y1 && (int64_t)t.x0 - t.dx >= 0 && (int64_t)t.x1 - t.dx <= w &&
           (int64_t)t.y0 - t.dy >= 0 && (int64_t)t.y1 - t.dy <= h && t.src_offset >= 0 &&
           t.src_offset <= src_bytes - h * w * 3;
}

// one layer's v for the lane's pixel k: `present` has bit t set for the tiles that are there
__device__ __forceinline__ Bgr layer_value(const adaisp_mosaic_layer& L, unsigned present, const uint8_t* __restrict__ src,
                                           uint64_t fx, uint64_t fy) {
    const Bgr pad = unpack_fill(L.fill);
    return tap_blend(fx, fy, [&](int64_t i, int64_t j) {
        int64_t at = -1;                          // scanned from the last tile down: the first that contains (i, j) wins
#pragma unroll
        for (int t = 3; t >= 0; --t) {
            const adaisp_mosaic_tile& T = L.tile[t];
            if (((present >> t) & 1u) && i >= T.x0 && i < T.x1 && j >= T.y0 && j < T.y1)
                at = T.src_offset + ((j - T.dy) * (int64_t)T.w + (i - T.dx)) * 3;
        }
        if (at < 0) return pad;
        const uint8_t* __restrict__ px = src + at;
        return Bgr{px[0], px[1], px[2]};
    });
}

__device__ __forceinline__ unsigned layer_tiles(const adaisp_mosaic_layer& L, int64_t src_bytes) {
    const int n = min(max(L.n_tiles, 0), 4);
    unsigned present = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (t < n && tile_present(L.tile[t], src_bytes)) present |= 1u << t;
    return present;
}

// TWO: the launch has images of two layers (n_layers = 2); without it the second layer's code is not there at all
template <bool VEC, bool TWO>
__global__ __launch_bounds__(AUG_THREADS) void k_mosaic_u8(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                           const adaisp_mosaic_desc* __restrict__ desc,
                                                           const uint8_t* __restrict__ luts, int n_luts,
                                                           uint8_t* __restrict__ dst, int S, int quads_per_row) {
    const adaisp_mosaic_desc& d = desc[blockIdx.y];
    warp_quads<VEC>(d.lut, luts, n_luts, dst, S, quads_per_row, [&](int x0, int y) {
        const adaisp_mosaic_layer &L0 = d.layer[0], &L1 = d.layer[1];
        const bool two = TWO && d.n_layers == 2;             // uniform over the workgroup
        const unsigned mix = (unsigned)min(max(d.mix, 0), 65536);
        const unsigned present0 = layer_tiles(L0, src_bytes), present1 = two ? layer_tiles(L1, src_bytes) : 0u;
        return [=, &L0, &L1, p0 = Q16Pos(L0.m, x0, y), p1 = two ? Q16Pos(L1.m, x0, y) : Q16Pos()]() mutable {
            Bgr v = layer_value(L0, present0, src, p0.fx, p0.fy);
            if (two) {
                const Bgr u = layer_value(L1, present1, src, p1.fx, p1.fy);
                v.b = (mix * v.b + (65536u - mix) * u.b) >> 16;
                v.g = (mix * v.g + (65536u - mix) * u.g) >> 16;
                v.r = (mix * v.r + (65536u - mix) * u.r) >> 16;
            }
            p0.step(), p1.step();
            return v;
        };
    });
}

// What the two entry points check and size alike, around the one launch that differs: `own` is the entry's own argument
// check, `launch(grid, quads_per_row, vec)` starts its kernel (vec: dword stores).
template <class Launch>
int launch_quads(const void* src, size_t src_bytes, const void* desc, const void* luts, int n_luts, const void* dst, int B,
                 int S, bool own, Launch launch) {
    if (!src || !desc || !dst || B < 1 || S < 1 || n_luts < 0 || (!luts && n_luts > 0)) return ADAISP_EINVAL;
    if (!own || src_bytes > (size_t)INT64_MAX) return ADAISP_EINVAL;
    if (B > 65535 || S > 32768) return ADAISP_ESHAPE;              // grid.y; pixel indices fit 32 bits
    const int qpr = (S + 3) / 4;
    const long quads = (long)S * qpr;
    launch(dim3((unsigned)((quads + AUG_THREADS - 1) / AUG_THREADS), (unsigned)B), qpr,
           (S % 4 == 0) && (reinterpret_cast<uintptr_t>(dst) % 4 == 0));
    return hipGetLastError() == hipSuccess ? ADAISP_OK : ADAISP_ELAUNCH;
}

}  // namespace
}  // namespace adaisp

extern "C" int adaisp_augment_u8(const uint8_t* src, size_t src_bytes, const adaisp_augment_desc* desc,
                                 const uint8_t* luts, int n_luts, uint8_t* dst, int B, int S, unsigned fill,
                                 void* stream) {
    using namespace adaisp;
    return launch_quads(src, src_bytes, desc, luts, n_luts, dst, B, S, fill <= 0xFFFFFFu, [&](dim3 grid, int qpr, bool vec) {
        hipLaunchKernelGGL(vec ? k_augment_u8<true> : k_augment_u8<false>, grid, dim3(AUG_THREADS), 0,
                           static_cast<hipStream_t>(stream), src, (int64_t)src_bytes, desc, luts, n_luts, dst, S, qpr, fill);
    });
}

extern "C" int adaisp_mosaic_u8(const uint8_t* src, size_t src_bytes, const adaisp_mosaic_desc* desc, const uint8_t* luts,
                                int n_luts, uint8_t* dst, int B, int S, int n_layers, void* stream) {
    using namespace adaisp;
    return launch_quads(src, src_bytes, desc, luts, n_luts, dst, B, S, n_layers == 1 || n_layers == 2,
                        [&](dim3 grid, int qpr, bool vec) {
        const auto kernel = n_layers == 2 ? (vec ? k_mosaic_u8<true, true> : k_mosaic_u8<false, true>)
                                          : (vec ? k_mosaic_u8<true, false> : k_mosaic_u8<false, false>);
        hipLaunchKernelGGL(kernel, grid, dim3(AUG_THREADS), 0, static_cast<hipStream_t>(stream), src, (int64_t)src_bytes,
                           desc, luts, n_luts, dst, S, qpr);
    });
}
