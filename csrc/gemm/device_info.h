// What the launch code asks the device, once: the CU count that sizes persistent and
// grid-striding grids (the GEMM's, the quantisers', the row kernels' of row_io.h).
#pragma once
#include <hip/hip_runtime.h>

namespace ddlb {

// The current device's CU count, read on first use and kept; 256 (an MI355X's) where the runtime
// does not say.
inline int num_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n <= 0)
      n = 256;
  }
  return n;
}

}  // namespace ddlb
