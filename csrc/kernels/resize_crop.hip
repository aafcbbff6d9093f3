// Device input pipeline, the ImageNet form: per-sample crop box resampled bilinearly to the output
// size (RandomResizedCrop / Resize + CenterCrop), horizontal flip, normalisation, the NHWC cast, the
// 3 -> 4 channel pad and mixup / cutmix, one read of the uint8 batch and one write of the model's
// input. The semantics are in api.h (resized_crop_batch); fluxmpi_amd/ops/augment.py holds the CPU
// reference that agrees bit for bit. The resampling is integer arithmetic with 11-bit weights; from
// the resampled byte on, the arithmetic is augment.hip's (augment_device.h).
//
// Shape. As in augment.hip a workgroup of 256 lanes owns up to 8 output rows of one sample
// (resize_crop_host.h: the geometry), stages source rows into LDS with aligned 16-byte global loads
// (the chunk that straddles either end of the batch is read bytewise, so no load leaves the tensor),
// and a lane then takes 8 output pixels and writes 48 or 64 bytes with 16-byte stores; w % 8 pixels
// and unaligned output addresses go pixel by pixel through the same arithmetic. Three phases, a
// barrier between them:
//
//   1. terms. The first lanes form the row terms (y0, y1, fy) of the workgroup's output rows and
//      decide what the LDS rows ("slots", 2 * rows per set) hold; all lanes form the column terms
//      (x0, x1 - x0, fx) of the output's w columns, the flip folded in. These are the only divisions:
//      two per output row and two per output column of a workgroup, none per pixel.
//   2. stage. The staged span of a source row is the sample's box: 3 * bw bytes from byte 3 * left.
//      Which rows: the R = nrows output rows need source rows y0(first) .. y1(last) of the box.
//        * union path: when that range has at most 2 * rows rows (always when bh <= 2 h), slot t
//          holds source row y0(first) + t: every source byte is read once per workgroup;
//        * pair path: otherwise (a reduction by more than 2) output row r's own pair y0(r), y1(r)
//          goes to slots 2 r, 2 r + 1; the rows between are never read.
//      The choice is per set and wave-uniform. Under cutmix the partner's set covers the rows of the
//      mixing box alone.
//   3. output. Per pixel and set two source pixels of each of the two rows, read as the 3 aligned LDS
//      dwords around their 6 bytes and shifted into place, the two-stage weighted sum in 24-bit
//      multiplies, then augment_device.h.
//
// A device box table forms addresses, so every box is clamped to the image before use. No atomics,
// no scratch, no host read: with a device block (aug_block_set) the launch is HIP-graph capturable.
//
// The products and sums are rounded separately (no fused multiply-add): contraction is off for this
// file (augment_device.h).
#include <stdexcept>
#include <string>

#include "../api.h"
#include "common.h"
#include "resize_crop_host.h"
// last: it turns contraction off for what follows
#include "augment_device.h"

namespace fluxmpi {
namespace {

static_assert(kRrcMaxRows == 8, "the slot tables below are indexed with shifts for 16 slots per set");
constexpr int kSlotShift = 4;  // log2(2 * kRrcMaxRows)

struct RrcArgs {
  const uint8_t* in;
  void* out;
  const int32_t* boxes;
  int64_t in_bytes;
  const uint32_t* dev_block;
  int B, H, W, h, w;
  uint32_t step;
  int mode, y0, x0, y1, x1;
  float lam;
  float a[3], b[3];
  int rows, slots, row_blocks, row_bytes, sets, wpad, row_tab, slot_tab, col_tab, stage, stage_shift, item_shift;
};

// a sample's box, clamped into the image (wave-uniform)
struct Box {
  int top, left, bh, bw, flip;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ Box box_of(const RrcArgs& k, int b) {
  const int32_t* __restrict__ t = k.boxes + 5 * static_cast<int64_t>(b);
  Box x;
  x.top = clampi(t[0], 0, k.H - 1);
  x.left = clampi(t[1], 0, k.W - 1);
  x.bh = clampi(t[2], 1, k.H - x.top);
  x.bw = clampi(t[3], 1, k.W - x.left);
  x.flip = t[4] & 1;
  return x;
}

// what an output row reads: the LDS byte offsets of the box's first byte in its two staged source
// rows, and fy
struct RowRd {
  int a, b;
  uint32_t fy;
};

__device__ __forceinline__ RowRd row_rd(const RrcArgs& k, const uint8_t* lds, int set, int r) {
  const uint32_t e = reinterpret_cast<const uint32_t*>(lds + k.row_tab)[set * kRrcMaxRows + r];
  const int32_t* slot = reinterpret_cast<const int32_t*>(lds + k.slot_tab) + (set << kSlotShift);
  const int sa = static_cast<int>(e & 0xffu), sb = static_cast<int>((e >> 8) & 0xffu);
  const int st = k.stage + set * k.slots * k.row_bytes;
  return {st + sa * k.row_bytes + (slot[sa] >> 16), st + sb * k.row_bytes + (slot[sb] >> 16), e >> 16};
}

// the two source pixels x0, x1 of one row as packed bytes (channel c at bits 8c): the 6 bytes from LDS
// byte `o` on, taken from the 3 aligned dwords around them (reads narrower than a dword at odd
// addresses are what this avoids); x1 = x0 (`far` == 0) or the next pixel (`far` == 24)
__device__ __forceinline__ void pixel_pair(const uint32_t* ldsw, int o, int far, uint32_t& p0, uint32_t& p1) {
  const uint32_t* q = ldsw + (o >> 2);
  const uint32_t sh = 8u * static_cast<uint32_t>(o & 3);
  const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
  const uint32_t w0 = __funnelshift_r(d0, d1, sh), w1 = __funnelshift_r(d1, d2, sh);  // bytes o .. o + 7
  p0 = w0;
  p1 = __funnelshift_r(w0, w1, static_cast<uint32_t>(far));
}

// the resampled pixel of one column entry (x0 | (x1 - x0) << 14 | fx << 15), packed: channel c at bits 8c
__device__ __forceinline__ uint32_t bilerp(const uint32_t* ldsw, const RowRd& r, uint32_t ce) {
  const int xo = 3 * static_cast<int>(ce & 0x3fffu);
  const int far = 24 * static_cast<int>((ce >> 14) & 1u);
  const uint32_t fx = ce >> 15, gx = 2048u - fx, gy = 2048u - r.fy;
  uint32_t a0, a1, b0, b1;
  pixel_pair(ldsw, r.a + xo, far, a0, a1);
  pixel_pair(ldsw, r.b + xo, far, b0, b1);
  uint32_t px = 0u;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int s = 8 * c;
    // every factor is below 2^24: the full-rate 24-bit multiply, not the quarter-rate 32-bit one
    const uint32_t t0 = __umul24((a0 >> s) & 0xffu, gx) + __umul24((a1 >> s) & 0xffu, fx);  // < 2^19
    const uint32_t t1 = __umul24((b0 >> s) & 0xffu, gx) + __umul24((b1 >> s) & 0xffu, fx);
    const uint32_t v = (__umul24(t0, gy) + __umul24(t1, r.fy) + (1u << 21)) >> 22;  // the sum is < 2^32
    px |= v << s;
  }
  return px;
}

template <typename T, int C, bool MIX>
__global__ __launch_bounds__(kRrcThreads) void resized_crop_kernel(RrcArgs k) {
  extern __shared__ uint4 rrc_lds[];
  uint8_t* lds = reinterpret_cast<uint8_t*>(rrc_lds);
  const uint32_t* ldsw = reinterpret_cast<const uint32_t*>(rrc_lds);
  const int tid = threadIdx.x;
  const int b = static_cast<int>(blockIdx.x) / k.row_blocks;
  const int i0 = (static_cast<int>(blockIdx.x) - b * k.row_blocks) * k.rows;
  const int nrows = k.h - i0 < k.rows ? k.h - i0 : k.rows;

  // MIX: the launch stages two sets (a mixing mode by value, or a device block that may select one)
  const Mix m = mix_of(k);
  const bool mixing = MIX && (m.mode == 1 || m.mode == 2);
  const int nsets = mixing ? 2 : 1;
  const int bp = k.B - 1 - b;
  const Box sb = box_of(k, b);
  const Box pb = mixing ? box_of(k, bp) : sb;
  const int64_t image = static_cast<int64_t>(k.H) * k.W * 3;
  const uint8_t* sbase = k.in + b * image;
  const uint8_t* pbase = k.in + bp * image;

  uint32_t* rowtab = reinterpret_cast<uint32_t*>(lds + k.row_tab);
  int32_t* slottab = reinterpret_cast<int32_t*>(lds + k.slot_tab);
  uint32_t* coltab = reinterpret_cast<uint32_t*>(lds + k.col_tab);

  // 1. terms: lane (set, sl) owns slot sl of its set; the even ones also own output row sl / 2
  if (tid < (nsets << kSlotShift)) {
    const int set = tid >> kSlotShift, sl = tid & ((1 << kSlotShift) - 1);
    const Box& bx = set ? pb : sb;
    int ra = i0, rb = i0 + nrows - 1;  // the output rows that read this set
    if (set == 1 && m.mode == 2) {
      ra = m.y0 > ra ? m.y0 : ra;
      if (m.y1 <= rb) rb = m.y1 > 0 ? m.y1 - 1 : -1;  // whatever a device block holds, nothing overflows
    }
    int entry = -1;
    if (sl < k.slots && ra <= rb) {
      const RrcTerm first = rrc_term(ra, bx.bh, k.h), last = rrc_term(rb, bx.bh, k.h);
      const bool uni = last.p1 - first.p0 < k.slots;
      const int r = sl >> 1, i = i0 + r;
      const bool mine = i >= ra && i <= rb;
      const RrcTerm t = rrc_term(mine ? i : ra, bx.bh, k.h);
      int y = -1;
      if (uni) {
        if (first.p0 + sl <= last.p1) y = first.p0 + sl;
      } else if (mine) {
        y = (sl & 1) ? t.p1 : t.p0;
      }
      if (y >= 0) {
        const int ay = bx.top + y;
        const uint32_t lo = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(set ? pbase : sbase)) +
                            static_cast<uint32_t>(ay * (3 * k.W) + 3 * bx.left);  // the low bits are all that count
        entry = ay | static_cast<int>((lo & 15u) << 16);
      }
      if (mine && !(sl & 1)) {
        const int s0 = uni ? t.p0 - first.p0 : sl, s1 = uni ? t.p1 - first.p0 : sl + 1;
        rowtab[set * kRrcMaxRows + r] = static_cast<uint32_t>(s0) | (static_cast<uint32_t>(s1) << 8) | (t.f << 16);
      }
    }
    slottab[tid] = entry;
  }
  for (int j = tid; j < k.w; j += kRrcThreads) {
    for (int set = 0; set < nsets; ++set) {
      const Box& bx = set ? pb : sb;
      const RrcTerm t = rrc_term(bx.flip ? k.w - 1 - j : j, bx.bw, k.w);
      coltab[set * k.wpad + j] = static_cast<uint32_t>(t.p0) | (static_cast<uint32_t>(t.p1 - t.p0) << 14) | (t.f << 15);
    }
  }
  __syncthreads();

  // 2. stage: the lanes walk (set, slot) x the row's chunks (resize_crop_host.h: stage_shift)
  {
    const int along = 1 << k.stage_shift;
    const int nsr = nsets * k.slots;
    for (int sr = tid >> k.stage_shift; sr < nsr; sr += kRrcThreads >> k.stage_shift) {
      const bool partner = sr >= k.slots;
      const int sl = partner ? sr - k.slots : sr;
      const int e = slottab[(partner ? 1 << kSlotShift : 0) + sl];
      if (e < 0) continue;
      const Box& bx = partner ? pb : sb;
      const int mis = e >> 16;
      const uint8_t* ga = (partner ? pbase : sbase) + ((e & 0xffff) * (3 * k.W) + 3 * bx.left) - mis;
      const int nch = (mis + 3 * bx.bw + 15) >> 4;
      uint8_t* lrow = lds + k.stage + static_cast<size_t>(sr) * k.row_bytes;
      for (int ck = tid & (along - 1); ck < nch; ck += along)
        *reinterpret_cast<uint4*>(lrow + 16 * ck) = load_chunk(k, ga + 16 * ck);
    }
  }
  __syncthreads();

  // 3. output: the lanes walk rows x the row's items (item_shift): w / 8 vector groups, then w % 8 pixels
  const int ngroups = k.w >> 3, per_row = ngroups + (k.w & 7);
  const int along = 1 << k.item_shift;
  T* __restrict__ out = static_cast<T*>(k.out);
  for (int r = tid >> k.item_shift; r < nrows; r += kRrcThreads >> k.item_shift) {
    const int i = i0 + r;
    const bool row_in = i >= m.y0 && i < m.y1;
    const bool use_p = mixing && (m.mode == 1 || row_in);
    const RowRd rs = row_rd(k, lds, 0, r);
    const RowRd rp = use_p ? row_rd(k, lds, 1, r) : rs;
    const uint32_t* cs = coltab;
    const uint32_t* cp = use_p ? coltab + k.wpad : coltab;
    T* orow = out + (static_cast<int64_t>(b) * k.h + i) * static_cast<int64_t>(k.w) * C;
    for (int q = tid & (along - 1); q < per_row; q += along) {
      if (q < ngroups) {
        const int j0 = 8 * q;
        uint32_t px[8], pp[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) px[t] = bilerp(ldsw, rs, cs[j0 + t]);
        if (use_p) {
#pragma unroll
          for (int t = 0; t < 8; ++t) pp[t] = bilerp(ldsw, rp, cp[j0 + t]);
        } else {
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
        const uint32_t px = bilerp(ldsw, rs, cs[j]);
        const uint32_t pp = use_p ? bilerp(ldsw, rp, cp[j]) : px;
        T o[C];
        pixel_out<T, C>(k, m, px, pp, use_p, row_in && j >= m.x0 && j < m.x1, o);
        T* dst = orow + static_cast<int64_t>(j) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) dst[c] = o[c];
      }
    }
  }
}

}  // namespace

void resized_crop_batch(const void* in, void* out, const int32_t* boxes, int64_t B, int H, int W, int h, int w, int C,
                        int dtype, const AugHyper& a, hipStream_t stream) {
  rrc_check(in, out, boxes, B, H, W, h, w, C, dtype == kBF16 || dtype == kF16, a);
  const RrcGeometry g = rrc_geometry(B, W, h, w, a.dev_block != nullptr || a.mode != 0);
  if (g.grid == 0) return;
  RrcArgs k{};
  k.in = static_cast<const uint8_t*>(in);
  k.out = out;
  k.boxes = boxes;
  k.in_bytes = B * H * static_cast<int64_t>(W) * 3;
  k.dev_block = a.dev_block;
  k.B = static_cast<int>(B), k.H = H, k.W = W, k.h = h, k.w = w;
  k.step = a.step;
  k.mode = a.mode, k.y0 = a.y0, k.x0 = a.x0, k.y1 = a.y1, k.x1 = a.x1, k.lam = a.lam;
  for (int c = 0; c < 3; ++c) k.a[c] = a.a[c], k.b[c] = a.b[c];
  k.rows = g.rows, k.slots = g.slots, k.row_blocks = g.row_blocks, k.row_bytes = g.row_bytes, k.sets = g.sets;
  k.wpad = g.wpad, k.row_tab = g.row_tab, k.slot_tab = g.slot_tab, k.col_tab = g.col_tab, k.stage = g.stage;
  k.stage_shift = g.stage_shift, k.item_shift = g.item_shift;
  dispatch_float(dtype, "resized_crop_batch: the output is bf16 or fp16", [&](auto tag) {
    using T = typename decltype(tag)::type;
    if constexpr (sizeof(T) == 2) {
      dispatch_int<3, 4>(C, "resized_crop_batch: channels must be 3 or 4", [&](auto c) {
        dispatch_bool(g.sets == 2, [&](auto mix) {
          resized_crop_kernel<T, decltype(c)::value, decltype(mix)::value>
              <<<static_cast<unsigned>(g.grid), kRrcThreads, g.lds_bytes, stream>>>(k);
        });
      });
    }
  });
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
