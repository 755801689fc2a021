// The image of a triangular inverse L^-T in MFMA B-fragment order: written by marg_image_kernel (blr_marginals.hpp), read by
// marginals_gemm_kernel and grad_gemm_kernel (blr_marginals.hpp), marginals_cols_kernel (blr_marg_multi.hpp) and loo_cols_kernel
// (blr_loo_multi.hpp).  Constants only, no kernel: every translation unit that touches the image includes this one statement of it.
#pragma once
#include "blr_common.hpp"

namespace blr {

constexpr int kPB = 128;  // panel / macro-tile edge (blr_large.hpp); the order of the factor one image covers

template <typename T>
struct MargGemmCfg {
  static constexpr int VEC = Mfma<T>::VEC;             // consecutive d per 16-byte load = MFMAs fed by one load
  static constexpr int NLOAD = kPB / (4 * VEC);        // loads per lane and tile: 16 (f64) / 8 (f32)
  static constexpr int NFRAG = 4 * 36;                 // B fragments of the image: sum_J 4 (J + 1)
  static constexpr int IMG_ELEMS = NFRAG * 64;
  static constexpr int OFF_MW = IMG_ELEMS * (int)sizeof(T);
  static constexpr int LDS_BYTES = OFF_MW + kPB * (int)sizeof(T);
  // contraction index of MFMA m (of a column block), lane group g = lane >> 4:  one 16-byte load covers VEC consecutive d
  __host__ __device__ static constexpr int d_of(int m, int g) { return 4 * VEC * (m / VEC) + VEC * g + (m % VEC); }
  __host__ __device__ static constexpr int frag0(int J) { return 2 * J * (J + 1); }  // first fragment of column block J
  // second image (gradient): groups of four fragments (Jc, J), J = Jc .. 7, in this order; first group of output block Jc
  __host__ __device__ static constexpr int frag2_0(int Jc) { return 8 * Jc - Jc * (Jc - 1) / 2; }
};

}  // namespace blr
