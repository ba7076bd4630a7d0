// ffpa_bwd_inst.hip — the attention backward of one padded head dim (-DFFPA_INST_D in {640, 768, 896, 1024}): the three kernels of ffpa_bwd_kernel.h, bf16 and
// fp16, and their launches on one stream.  A head dim in between runs here with d_valid < D: the missing columns are zero fragments and are never stored.
#define FFPA_BWD_KERNELS 1
#include "ffpa_bwd_kernel.h"
#include "ffpa_launch_kernel.h"

#ifndef FFPA_INST_D
#error "ffpa_bwd_inst.hip is compiled once per padded head dim: -DFFPA_INST_D=<640 | 768 | 896 | 1024>"
#endif

namespace ffpa {

namespace {
template <typename T, int D>
int launch_bwd(const BwdArgs& a, hipStream_t stream) {
  static_assert(bwd_dkdv_lds_bytes(D) <= 160 * 1024 && bwd_dq_lds_bytes(D) <= 160 * 1024, "the images and the exchange area fit the LDS");
  const int64_t rows = (int64_t)a.B * a.Hq * a.NqP;
  int st = launch_kernel<bwd::ffpa_bwd_delta_kernel<T>>((int)((rows + 3) / 4), 0, stream, a);
  if (st != 0) return st;
  const int kt = (a.Nkv + kBwdKeysDkdv - 1) / kBwdKeysDkdv;
  st = launch_kernel<bwd::ffpa_bwd_dkdv_kernel<T, D>>(a.B * a.Hkv * kt, bwd_dkdv_lds_bytes(D), stream, a);
  if (st != 0) return st;
  return launch_kernel<bwd::ffpa_bwd_dq_kernel<T, D>>(a.B * a.Hq * (a.NqP / kBwdRows), bwd_dq_lds_bytes(D), stream, a);
}
}  // namespace

#define FFPA_BWD_CAT_(a, b) a##b
#define FFPA_BWD_CAT(a, b) FFPA_BWD_CAT_(a, b)
int FFPA_BWD_CAT(launch_bwd_d, FFPA_INST_D)(const BwdArgs& a, hipStream_t stream) {
  if (a.fp16) return launch_bwd<_Float16, FFPA_INST_D>(a, stream);
  return launch_bwd<__bf16, FFPA_INST_D>(a, stream);
}

}  // namespace ffpa
