// Device input pipeline: random crop (with zero-extension), horizontal flip, normalisation, the
// NHWC cast, the 3 -> 4 channel pad and mixup / cutmix, one read of the uint8 batch and one write of
// the model's input. The semantics are in api.h (augment_batch); fluxmpi_amd/ops/augment.py holds
// the CPU reference that agrees bit for bit.
//
// Shape. The kernel is bandwidth-bound and the work is in the loads: a crop's rows start at
// arbitrary bytes (3 * ox into a row of 3 W bytes of a batch whose base is itself unaligned). A
// workgroup of 256 lanes owns up to 8 output rows of one sample (augment_host.h: the geometry; the
// lanes walk rows x a power of two of lanes along a row, so no lane divides). It
// stages the source span of each row, and of the partner's row when mixing, into LDS with aligned
// 16-byte global loads (the chunk that straddles either end of the batch is read bytewise, so no load
// leaves the tensor). Then a lane takes 8 output pixels: 7 aligned LDS dwords around its 24 source
// bytes, shifted into place, in either direction (a flip reverses the 8 pixels in registers), and
// writes 48 or 64 bytes with 16-byte stores. Pixels that the vector path does not cover (w % 8, a
// group that reaches over the image edge, an output address that is not 16-byte aligned) go pixel by
// pixel through the same arithmetic, so both paths give the same bits. No atomics, no scratch, no
// host read: with a device block (aug_block_set) the launch is HIP-graph capturable.
//
// The products and sums are rounded separately (no fused multiply-add): contraction is off for this
// file.
#include <stdexcept>
#include <string>

#include "../api.h"
#include "augment_host.h"
#include "common.h"
#include "optim_sr.h"
// last: it turns contraction off for what follows
#include "augment_device.h"

#pragma clang fp contract(off)

namespace fluxmpi {
namespace {

struct AugArgs {
  const uint8_t* in;
  void* out;
  int64_t in_bytes;
  int64_t sample_offset;
  const uint32_t* dev_block;
  int B, H, W, h, w;
  uint32_t rx, ry;
  uint32_t key0, key1, stream, step;
  int pad, fill, crop_center, flip;
  int mode, y0, x0, y1, x1;
  float lam;
  float a[3], b[3];
  int rows, row_blocks, row_bytes, chunks, sets, stage_shift, item_shift;
};

// a sample's draws: source pixel of output (i, j) = (i + oy, (flip ? w - 1 - j : j) + ox)
struct Sample {
  const uint8_t* base;  // the sample's first byte
  int ox, oy, flip;
};

__device__ __forceinline__ Sample sample_of(const AugArgs& k, int b, uint32_t step) {
  Sample s{k.in + static_cast<int64_t>(b) * k.H * k.W * 3, 0, 0, 0};
  if (k.crop_center) {
    s.ox = static_cast<int>((k.rx - 1) / 2);
    s.oy = static_cast<int>((k.ry - 1) / 2);
  } else {
    const uint64_t n = static_cast<uint64_t>(k.sample_offset + b);
    const Philox4 p = philox4x32_10(static_cast<uint32_t>(n), static_cast<uint32_t>(n >> 32), k.stream, step, k.key0,
                                    k.key1);
    s.ox = static_cast<int>(__umulhi(p.w[0], k.rx));
    s.oy = static_cast<int>(__umulhi(p.w[1], k.ry));
    s.flip = k.flip ? static_cast<int>(p.w[2] & 1u) : 0;
  }
  s.ox -= k.pad;
  s.oy -= k.pad;
  return s;
}

// the part of output row i's source row that lies in the image: columns [c0, c0 + n) of one source
// row, as staged: `mis` bytes into the first of `nch` aligned 16-byte chunks from `ga`
struct RowSrc {
  bool ok;
  int c0, n, mis, nch;
  const uint8_t* ga;
};

__device__ __forceinline__ RowSrc row_src(const AugArgs& k, const Sample& s, int i) {
  RowSrc r{};
  const int sr = i + s.oy;
  const int c0 = s.ox > 0 ? s.ox : 0;
  const int c1 = s.ox + k.w < k.W ? s.ox + k.w : k.W;
  r.ok = sr >= 0 && sr < k.H && c1 > c0;
  if (!r.ok) return r;
  r.c0 = c0;
  r.n = c1 - c0;
  const uint8_t* g0 = s.base + (static_cast<int64_t>(sr) * (3 * k.W) + 3 * c0);  // 3 W < 2^26: one 32 x 32 -> 64
  r.mis = static_cast<int>(reinterpret_cast<uintptr_t>(g0) & 15u);
  r.ga = g0 - r.mis;
  r.nch = (r.mis + 3 * r.n + 15) >> 4;
  return r;
}

__device__ __forceinline__ void stage_row(const AugArgs& k, const RowSrc& r, uint8_t* lrow, int ck) {
  if (r.ok && ck < r.nch) *reinterpret_cast<uint4*>(lrow + 16 * ck) = load_chunk(k, r.ga + 16 * ck);
}

// one pixel's three bytes, packed (channel c at bits 8c), of output column j
__device__ __forceinline__ uint32_t pixel_bytes(const AugArgs& k, const Sample& s, const RowSrc& r,
                                                const uint8_t* lrow, int j) {
  const int col = (s.flip ? k.w - 1 - j : j) + s.ox;
  if (!r.ok || col < r.c0 || col >= r.c0 + r.n) return static_cast<uint32_t>(k.fill) * 0x010101u;
  const uint8_t* q = lrow + r.mis + 3 * (col - r.c0);
  return static_cast<uint32_t>(q[0]) | (static_cast<uint32_t>(q[1]) << 8) | (static_cast<uint32_t>(q[2]) << 16);
}

// the packed pixels of output columns j0 .. j0 + 7
__device__ __forceinline__ void group_bytes(const AugArgs& k, const Sample& s, const RowSrc& r, const uint8_t* lrow,
                                            int j0, uint32_t (&px)[8]) {
  const int cs = (s.flip ? k.w - 8 - j0 : j0) + s.ox;  // leftmost source column of the group
  if (r.ok && cs >= r.c0 && cs + 8 <= r.c0 + r.n) {
    const int o = r.mis + 3 * (cs - r.c0);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(lrow + (o & ~3));
    const int sh = 8 * (o & 3);
    uint32_t d[7];
#pragma unroll
    for (int t = 0; t < 7; ++t) d[t] = q[t];
    uint32_t e[7];  // the 24 bytes from o on, as dwords (e[6] pads the last funnel)
#pragma unroll
    for (int t = 0; t < 6; ++t)
      e[t] = static_cast<uint32_t>(((static_cast<uint64_t>(d[t + 1]) << 32) | d[t]) >> sh);
    e[6] = 0u;
    uint32_t src[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int byte = 3 * t, wd = byte >> 2, bs = 8 * (byte & 3);
      src[t] = static_cast<uint32_t>(((static_cast<uint64_t>(e[wd + 1]) << 32) | e[wd]) >> bs) & 0xffffffu;
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) px[t] = s.flip ? src[7 - t] : src[t];
  } else {
#pragma unroll
    for (int t = 0; t < 8; ++t) px[t] = pixel_bytes(k, s, r, lrow, j0 + t);
  }
}

template <typename T, int C, bool MIX>
__global__ __launch_bounds__(kAugThreads) void augment_kernel(AugArgs k) {
  extern __shared__ uint4 aug_lds[];
  uint8_t* lds = reinterpret_cast<uint8_t*>(aug_lds);
  const int tid = threadIdx.x;
  const int b = static_cast<int>(blockIdx.x) / k.row_blocks;
  const int i0 = (static_cast<int>(blockIdx.x) - b * k.row_blocks) * k.rows;
  const int nrows = k.h - i0 < k.rows ? k.h - i0 : k.rows;

  // MIX: the launch stages two sets (a mixing mode by value, or a device block that may select one)
  const Mix m = mix_of(k);
  const bool mixing = MIX && (m.mode == 1 || m.mode == 2);
  const Sample s = sample_of(k, b, m.step);
  const Sample p = mixing ? sample_of(k, k.B - 1 - b, m.step) : s;

  // stage: the lanes walk (set, row) x the row's chunks (augment_host.h: stage_shift)
  {
    const int along = 1 << k.stage_shift;
    const int nsr = mixing ? 2 * nrows : nrows;
    for (int sr = tid >> k.stage_shift; sr < nsr; sr += kAugThreads >> k.stage_shift) {
      const bool partner = sr >= nrows;
      const int r = partner ? sr - nrows : sr;
      const int i = i0 + r;
      if (partner && !(m.mode == 1 || (i >= m.y0 && i < m.y1))) continue;  // cutmix reads the box's rows alone
      const RowSrc rs = row_src(k, partner ? p : s, i);
      uint8_t* lrow = lds + static_cast<size_t>((partner ? k.rows : 0) + r) * k.row_bytes;
      for (int ck = tid & (along - 1); ck < k.chunks; ck += along) stage_row(k, rs, lrow, ck);
    }
  }
  __syncthreads();

  // output: the lanes walk rows x the row's items (item_shift): w / 8 vector groups, then w % 8 pixels
  const int ngroups = k.w >> 3, per_row = ngroups + (k.w & 7);
  const int along = 1 << k.item_shift;
  T* __restrict__ out = static_cast<T*>(k.out);
  for (int r = tid >> k.item_shift; r < nrows; r += kAugThreads >> k.item_shift) {
    const int i = i0 + r;
    const uint8_t* lrow = lds + static_cast<size_t>(r) * k.row_bytes;
    const uint8_t* prow = lds + static_cast<size_t>(k.rows + r) * k.row_bytes;
    const RowSrc rs = row_src(k, s, i);
    const bool row_in = i >= m.y0 && i < m.y1;
    const bool use_p = mixing && (m.mode == 1 || row_in);
    const RowSrc rp = use_p ? row_src(k, p, i) : rs;
    T* orow = out + (static_cast<int64_t>(b) * k.h + i) * static_cast<int64_t>(k.w) * C;
    for (int q = tid & (along - 1); q < per_row; q += along) {
      if (q < ngroups) {
        const int j0 = 8 * q;
        uint32_t px[8], pp[8];
        group_bytes(k, s, rs, lrow, j0, px);
        if (use_p) group_bytes(k, p, rp, prow, j0, pp);
        else {
#pragma unroll
          for (int t = 0; t < 8; ++t) pp[t] = px[t];
        }
        union {
          T e[8 * C];
          uint4 v[C];
        } o;
#pragma unroll
        for (int t = 0; t < 8; ++t)
          pixel_out<T, C>(k, m, px[t], pp[t], use_p, row_in && j0 + t >= m.x0 && j0 + t < m.x1, o.e + C * t);
        T* dst = orow + static_cast<int64_t>(j0) * C;
        if (aligned16(dst)) {
#pragma unroll
          for (int t = 0; t < C; ++t) reinterpret_cast<uint4*>(dst)[t] = o.v[t];
        } else {
#pragma unroll
          for (int t = 0; t < 8 * C; ++t) dst[t] = o.e[t];
        }
      } else {
        const int j = 8 * ngroups + (q - ngroups);
        const uint32_t px = pixel_bytes(k, s, rs, lrow, j);
        const uint32_t pp = use_p ? pixel_bytes(k, p, rp, prow, j) : px;
        T o[C];
        pixel_out<T, C>(k, m, px, pp, use_p, row_in && j >= m.x0 && j < m.x1, o);
        T* dst = orow + static_cast<int64_t>(j) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) dst[c] = o[c];
      }
    }
  }
}

__global__ void aug_block_set_kernel(uint32_t* __restrict__ blk, uint32_t step, int mode, int y0, int x0, int y1,
                                     int x1, float lam) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  blk[kAugStep] = step;
  blk[kAugMode] = static_cast<uint32_t>(mode);
  blk[kAugY0] = static_cast<uint32_t>(y0);
  blk[kAugX0] = static_cast<uint32_t>(x0);
  blk[kAugY1] = static_cast<uint32_t>(y1);
  blk[kAugX1] = static_cast<uint32_t>(x1);
  blk[kAugLam] = __builtin_bit_cast(uint32_t, lam);
  blk[7] = 0u;
}

}  // namespace

void augment_batch(const void* in, void* out, int64_t B, int H, int W, int h, int w, int C, int dtype,
                   const AugHyper& a, hipStream_t stream) {
  aug_check(in, out, B, H, W, h, w, C, dtype == kBF16 || dtype == kF16, a);
  const AugGeometry g = aug_geometry(B, W, h, w, a.dev_block != nullptr || a.mode != 0);
  if (g.grid == 0) return;
  AugArgs k{};
  k.in = static_cast<const uint8_t*>(in);
  k.out = out;
  k.in_bytes = B * H * static_cast<int64_t>(W) * 3;
  k.sample_offset = a.sample_offset;
  k.dev_block = a.dev_block;
  k.B = static_cast<int>(B), k.H = H, k.W = W, k.h = h, k.w = w;
  k.rx = static_cast<uint32_t>(W + 2 * a.pad - w + 1);
  k.ry = static_cast<uint32_t>(H + 2 * a.pad - h + 1);
  k.key0 = static_cast<uint32_t>(a.seed), k.key1 = static_cast<uint32_t>(a.seed >> 32);
  k.stream = a.stream, k.step = a.step;
  k.pad = a.pad, k.fill = a.fill, k.crop_center = a.crop_center, k.flip = a.flip;
  k.mode = a.mode, k.y0 = a.y0, k.x0 = a.x0, k.y1 = a.y1, k.x1 = a.x1, k.lam = a.lam;
  for (int c = 0; c < 3; ++c) k.a[c] = a.a[c], k.b[c] = a.b[c];
  k.rows = g.rows, k.row_blocks = g.row_blocks, k.row_bytes = g.row_bytes, k.chunks = g.chunks, k.sets = g.sets;
  k.stage_shift = g.stage_shift, k.item_shift = g.item_shift;
  dispatch_float(dtype, "augment_batch: the output is bf16 or fp16", [&](auto tag) {
    using T = typename decltype(tag)::type;
    if constexpr (sizeof(T) == 2) {
      dispatch_int<3, 4>(C, "augment_batch: channels must be 3 or 4", [&](auto c) {
        dispatch_bool(g.sets == 2, [&](auto mix) {
          augment_kernel<T, decltype(c)::value, decltype(mix)::value>
              <<<static_cast<unsigned>(g.grid), kAugThreads, g.lds_bytes, stream>>>(k);
        });
      });
    }
  });
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

void aug_block_set(void* block, uint32_t step, int mode, int y0, int x0, int y1, int x1, float lam,
                   hipStream_t stream) {
  if (block == nullptr) throw std::runtime_error("aug_block_set: needs the block");
  if (mode < 0 || mode > 2) throw std::runtime_error("aug_block_set: mode must be 0, 1 or 2");
  aug_block_set_kernel<<<1, 64, 0, stream>>>(static_cast<uint32_t*>(block), step, mode, y0, x0, y1, x1, lam);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
