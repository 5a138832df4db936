// Resident form of the split-MFMA fused flow kernel (flow_kernel_x3r,
// zf_flow_x3_kernel.h), K = 16 knots: swish couplings with two transformed
// dims, forward and inverse / sample — the shapes that measured faster than
// the streaming form (profiles/resident_ab.txt), each with the generic frame
// and with the frame specialised for D = 4, C = 0, affine ShiftBounds and a
// Normal latent (profiles/resident_frame_ab.txt).  Every other shape stays on
// the streaming form (x3_resident_fits).
#include "zf_flow_x3_kernel.h"

namespace zf {

int launch_x3r_k16(const X3Launch& a, bool inverse) { return launch_x3r<16, false>(a, inverse); }

}  // namespace zf

#ifdef ZF_X3_TRACE
// tuning build only: install the stamp buffer of the resident kernels (n stamps of 8 bytes; null: no stamps)
extern "C" int zf_x3r_trace_set_k16(void* buf, long long n) {
  if (hipMemcpyToSymbol(HIP_SYMBOL(zf::x3r_trace_buf), &buf, sizeof(buf)) != hipSuccess) return 1;
  return hipMemcpyToSymbol(HIP_SYMBOL(zf::x3r_trace_cap), &n, sizeof(n)) == hipSuccess ? 0 : 1;
}
#endif
