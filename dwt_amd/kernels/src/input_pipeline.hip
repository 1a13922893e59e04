// Device-side input pipeline for MI355X (gfx950): resized uint8 HWC frames
// -> the (source, target, target_aug) training batch, in the model's dtype
// and in NHWC, in one launch.
//
// Per output image n a host-drawn table names the frame and the view:
//   src_index[n], top[n], left[n]   which frame, where the crop starts
//   flags[n]                        bit 0 = horizontal flip, bit 1 = affine
//   inv_affine[n][4]                inverse of the forward 2x2 matrix, acting
//                                   on (row, col) indices
// and the kernel applies, in the loaders' order (RandomCrop, flip, ToTensor,
// random affine, Normalize):
//   crop(r, c) = images[src, top + r, left + (flip ? cw-1-c : c), :] / 255
//   plain :  out = (crop(r, c) - mean) / std
//   affine:  p = inv_affine . (r, c); outside [0, ch-1] x [0, cw-1] the
//            sample is 0 (scipy mode="constant", cval=0: the edge itself is
//            inside and nothing is interpolated beyond it), otherwise the
//            bilinear interpolation of crop; then the same normalization, so
//            out-of-frame pixels come out as (0 - mean) / std.
//
// Normalization is affine in the sample, so the kernel keeps samples in
// uint8 units and applies one fma per element with scale = 1 / (255 std) and
// bias = -mean / std; everything is fp32 and rounded once at the store.
//
// Pure streaming kernel (cdna_hip_programming.md Guideline 13) over the
// flattened NHWC output.  16-B chunks (8 bf16 / 4 fp32) straddle pixels, rows
// and images when C = 3, but three chunks hold exactly VW whole pixels and
// every image starts on a pixel, so each lane owns VW consecutive pixels of
// the flattened batch = three 16-B stores: it decodes its first pixel once and
// walks (col, row, image) from there.  A group inside one image — nearly all
// of them — takes a branch-free path that issues all its loads before the
// first use: a plain group inside one crop row is one 3*VW-byte block read
// (unaligned dword loads, mirrored under flip), an affine pixel reads its
// four taps as two 6-byte pixel pairs.  A group that straddles two images
// walks pixel by pixel.  The pixels past the last whole group are written one
// per lane, with scalar stores, by the lanes after the vector body — same
// launch, no atomics, no LDS.  Measured: profiles/input_pipeline.md.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dwtin {

#define DEV_INLINE __device__ __forceinline__

struct ViewParams {
  const uint8_t* images;      // [N_in, Hs, Ws, 3]
  const int* src_index;       // [N_out]
  const int* top;
  const int* left;
  const int* flags;
  const float* inv_affine;    // [N_out, 4]
  int N_in, Hs, Ws;
  int ch, cw;
  int ppi;                    // pixels per output image, ch * cw
  int64_t total_px;           // N_out * ppi
  int64_t n_groups;           // whole groups of VW pixels
  float scale[3], bias[3];
};

// one output image's view, read once per lane per image it touches
struct Row {
  const uint8_t* base;        // &images[src, top, left, 0]
  bool flip, affine;
  float a00, a01, a10, a11;
};

DEV_INLINE Row load_row(const ViewParams& p, int64_t n) {
  Row r;
  // the table is validated on the host; the clamps only keep a corrupt table
  // from reading outside the frames
  const int src = min(max(p.src_index[n], 0), p.N_in - 1);
  const int top = min(max(p.top[n], 0), p.Hs - p.ch);
  const int left = min(max(p.left[n], 0), p.Ws - p.cw);
  const int fl = p.flags[n];
  r.base = p.images + (((int64_t)src * p.Hs + top) * p.Ws + left) * 3;
  r.flip = fl & 1;
  r.affine = fl & 2;
  const float4 a = *reinterpret_cast<const float4*>(p.inv_affine + 4 * n);
  r.a00 = a.x; r.a01 = a.y; r.a10 = a.z; r.a11 = a.w;
  return r;
}

// crop(r, c) in uint8 units, three channels; 0 <= r < ch, 0 <= c < cw
DEV_INLINE void crop_px(const ViewParams& p, const Row& row, int r, int c,
                        float v[3]) {
  const int cc = row.flip ? p.cw - 1 - c : c;
  const uint8_t* q = row.base + (r * p.Ws + cc) * 3;   // < Hs*Ws*3 < 2^31
  v[0] = (float)q[0]; v[1] = (float)q[1]; v[2] = (float)q[2];
}

// crop(r, c .. c+NP-1) for c + NP <= cw: the NP pixels are 3*NP consecutive
// bytes of one frame row (mirrored under flip), read as one unaligned block
// so the compiler can use dword loads instead of 3*NP byte loads.
template <int NP>
DEV_INLINE void crop_run(const ViewParams& p, const Row& row, int r, int c,
                         float* v) {
  const int c_lo = row.flip ? p.cw - c - NP : c;
  uint8_t b[3 * NP];
  __builtin_memcpy(b, row.base + (r * p.Ws + c_lo) * 3, 3 * NP);
#pragma unroll
  for (int j = 0; j < NP; ++j) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      v[3 * j + k] = row.flip ? (float)b[3 * (NP - 1 - j) + k]
                              : (float)b[3 * j + k];
  }
}

// the affine view's sample at output pixel (r, c), in uint8 units.  Branch
// free: the taps of a clamped coordinate are always read and an outside
// pixel is zeroed by a select, so the loads of a group can all be in flight.
DEV_INLINE void affine_px(const ViewParams& p, const Row& row, int r, int c,
                          float v[3]) {
  const float pr = row.a00 * (float)r + row.a01 * (float)c;
  const float pc = row.a10 * (float)r + row.a11 * (float)c;
  const float rmax = (float)(p.ch - 1), cmax = (float)(p.cw - 1);
  // written so that a NaN coordinate is outside too
  const bool inside = pr >= 0.f && pr <= rmax && pc >= 0.f && pc <= cmax;
  const float qr = fminf(fmaxf(pr, 0.f), rmax);   // == pr when inside
  const float qc = fminf(fmaxf(pc, 0.f), cmax);
  const int r0 = (int)qr, c0 = (int)qc;            // >= 0: trunc == floor
  const float fr = qr - (float)r0, fc = qc - (float)c0;
  const int r1 = min(r0 + 1, p.ch - 1);
  float v00[3], v01[3], v10[3], v11[3];
  if (p.cw >= 2) {                                 // uniform
    // the taps (c0, c1 = min(c0 + 1, cw - 1)) lie in the pixel pair
    // (c_lo, c_lo + 1): one 6-byte run per row.  At c0 == cw - 1 both taps
    // are the pair's second pixel (and fc == 0).
    const int c_lo = min(c0, p.cw - 2);
    float t[6], u[6];
    crop_run<2>(p, row, r0, c_lo, t);
    crop_run<2>(p, row, r1, c_lo, u);
    const bool second = c0 != c_lo;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v00[k] = second ? t[3 + k] : t[k];
      v01[k] = t[3 + k];
      v10[k] = second ? u[3 + k] : u[k];
      v11[k] = u[3 + k];
    }
  } else {
    crop_px(p, row, r0, 0, v00);
    crop_px(p, row, r1, 0, v10);
#pragma unroll
    for (int k = 0; k < 3; ++k) { v01[k] = v00[k]; v11[k] = v10[k]; }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float t0 = v00[k] + fc * (v01[k] - v00[k]);
    const float t1 = v10[k] + fc * (v11[k] - v10[k]);
    v[k] = inside ? t0 + fr * (t1 - t0) : 0.f;
  }
}

DEV_INLINE void sample_px(const ViewParams& p, const Row& row, int r, int c,
                          float v[3]) {
  if (row.affine) affine_px(p, row, r, c, v);
  else crop_px(p, row, r, c, v);
}

DEV_INLINE unsigned int bf16_bits(float f) {
  union { unsigned int u; float f; } v;
  v.f = f;
  // round-to-nearest-even like PyTorch's float->bf16 (values are finite)
  return (v.u + 0x7fffu + ((v.u >> 16) & 1u)) >> 16;
}

DEV_INLINE void store_chunk(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
DEV_INLINE void store_chunk(c10::BFloat16* p, const float* v) {
  *reinterpret_cast<uint4*>(p) =
      make_uint4(bf16_bits(v[0]) | (bf16_bits(v[1]) << 16),
                 bf16_bits(v[2]) | (bf16_bits(v[3]) << 16),
                 bf16_bits(v[4]) | (bf16_bits(v[5]) << 16),
                 bf16_bits(v[6]) | (bf16_bits(v[7]) << 16));
}
DEV_INLINE void store_one(float* p, float v) { *p = v; }
DEV_INLINE void store_one(c10::BFloat16* p, float v) {
  *reinterpret_cast<unsigned short*>(p) = (unsigned short)bf16_bits(v);
}

template <typename T>
__global__ void __launch_bounds__(256)
assemble_views_kernel(ViewParams p, T* __restrict__ out) {
  constexpr int VW = 16 / sizeof(T);     // pixels per group, elements per chunk
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // lanes [0, n_groups) own a group each, the lanes after them one tail pixel
  const bool vec = t < p.n_groups;
  const int64_t px0 = vec ? t * VW : p.n_groups * VW + (t - p.n_groups);
  if (px0 >= p.total_px) return;

  int64_t n;
  int rem;
  if (p.total_px < ((int64_t)1 << 31)) {   // uniform: 32-bit divide
    const unsigned q = (unsigned)px0 / (unsigned)p.ppi;
    n = q;
    rem = (int)((unsigned)px0 - q * (unsigned)p.ppi);
  } else {
    n = px0 / p.ppi;
    rem = (int)(px0 - n * p.ppi);
  }
  int r = rem / p.cw;
  int c = rem - r * p.cw;
  Row row = load_row(p, n);
  T* o = out + px0 * 3;

  if (!vec) {
    float s[3];
    sample_px(p, row, r, c, s);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      store_one(o + k, fmaf(s[k], p.scale[k], p.bias[k]));
    return;
  }

  float s[VW * 3];
  if (rem + VW > p.ppi) {
    // the group runs into image n + 1 (px0 + VW <= total_px: n + 1 < N_out)
    for (int j = 0; j < VW; ++j) {
      sample_px(p, row, r, c, s + 3 * j);
      if (++c == p.cw) {
        c = 0;
        if (++r == p.ch && j + 1 < VW) {
          r = 0;
          row = load_row(p, ++n);
        }
      }
    }
  } else if (row.affine) {
    // inside image n: branch-free walk, every load issued before the first use
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      affine_px(p, row, r, c, s + 3 * j);
      const bool wrap = ++c == p.cw;
      c = wrap ? 0 : c;
      r = (wrap && j + 1 < VW) ? r + 1 : r;
    }
  } else if (c + VW <= p.cw) {
    crop_run<VW>(p, row, r, c, s);       // inside one row: one block read
  } else {
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      crop_px(p, row, r, c, s + 3 * j);
      const bool wrap = ++c == p.cw;
      c = wrap ? 0 : c;
      r = (wrap && j + 1 < VW) ? r + 1 : r;
    }
  }

#pragma unroll
  for (int j = 0; j < VW * 3; ++j)
    s[j] = fmaf(s[j], p.scale[j % 3], p.bias[j % 3]);
  store_chunk(o, s);
  store_chunk(o + VW, s + VW);
  store_chunk(o + 2 * VW, s + 2 * VW);
}

}  // namespace dwtin

void assemble_views(torch::Tensor images, torch::Tensor src_index,
                    torch::Tensor top, torch::Tensor left, torch::Tensor flags,
                    torch::Tensor inv_affine, torch::Tensor out,
                    std::vector<double> mean, std::vector<double> std_) {
  TORCH_CHECK(images.is_cuda() && images.scalar_type() == torch::kUInt8 &&
              images.dim() == 4 && images.size(3) == 3 &&
              images.is_contiguous(),
              "assemble_views: images must be contiguous uint8 [N, H, W, 3] on the GPU");
  TORCH_CHECK(out.is_cuda() && out.dim() == 4 && out.size(1) == 3 &&
              out.is_contiguous(at::MemoryFormat::ChannelsLast),
              "assemble_views: out must be channels_last [N, 3, ch, cw] on the GPU");
  TORCH_CHECK(out.get_device() == images.get_device(),
              "assemble_views: images and out on different devices");
  const int64_t n_out = out.size(0);
  for (const torch::Tensor* t : {&src_index, &top, &left, &flags}) {
    TORCH_CHECK(t->is_cuda() && t->get_device() == images.get_device() &&
                t->scalar_type() == torch::kInt32 && t->dim() == 1 &&
                t->size(0) == n_out && t->is_contiguous(),
                "assemble_views: per-row tables must be contiguous int32 [N_out] on the GPU");
  }
  TORCH_CHECK(inv_affine.is_cuda() &&
              inv_affine.get_device() == images.get_device() &&
              inv_affine.scalar_type() == torch::kFloat32 &&
              inv_affine.numel() == 4 * n_out && inv_affine.is_contiguous() &&
              reinterpret_cast<uintptr_t>(inv_affine.data_ptr()) % 16 == 0,
              "assemble_views: inv_affine must be contiguous, 16-B aligned fp32 [N_out, 4] on the GPU");
  TORCH_CHECK(mean.size() == 3 && std_.size() == 3,
              "assemble_views: mean and std take three values each");
  const int64_t ch = out.size(2), cw = out.size(3);
  TORCH_CHECK(images.size(0) >= 1 && ch >= 1 && cw >= 1 &&
              ch <= images.size(1) && cw <= images.size(2),
              "assemble_views: crop does not fit the frames");
  TORCH_CHECK(images.size(1) * images.size(2) * 3 < (int64_t)1 << 31,
              "assemble_views: frame too large");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0,
              "assemble_views: out must be 16-B aligned");
  if (n_out == 0) return;

  dwtin::ViewParams p;
  p.images = images.data_ptr<uint8_t>();
  p.src_index = src_index.data_ptr<int>();
  p.top = top.data_ptr<int>();
  p.left = left.data_ptr<int>();
  p.flags = flags.data_ptr<int>();
  p.inv_affine = inv_affine.data_ptr<float>();
  p.N_in = (int)images.size(0);
  p.Hs = (int)images.size(1);
  p.Ws = (int)images.size(2);
  p.ch = (int)ch;
  p.cw = (int)cw;
  p.ppi = (int)(ch * cw);
  p.total_px = n_out * ch * cw;
  for (int k = 0; k < 3; ++k) {
    TORCH_CHECK(std_[k] != 0.0, "assemble_views: std must be non-zero");
    p.scale[k] = (float)(1.0 / (255.0 * std_[k]));
    p.bias[k] = (float)(-mean[k] / std_[k]);
  }

  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  auto launch = [&](auto* optr) {
    using T = std::remove_pointer_t<decltype(optr)>;
    constexpr int VW = 16 / sizeof(T);
    p.n_groups = p.total_px / VW;
    const int64_t lanes = p.n_groups + (p.total_px - p.n_groups * VW);
    const int64_t blocks = (lanes + 255) / 256;
    TORCH_CHECK(blocks < (int64_t)1 << 31, "assemble_views: batch too large");
    hipLaunchKernelGGL((dwtin::assemble_views_kernel<T>), dim3(blocks),
                       dim3(256), 0, stream, p, optr);
  };
  if (out.scalar_type() == torch::kFloat32) {
    launch(out.data_ptr<float>());
  } else if (out.scalar_type() == torch::kBFloat16) {
    launch(out.data_ptr<c10::BFloat16>());
  } else {
    TORCH_CHECK(false, "assemble_views: out must be fp32 or bf16");
  }
}
