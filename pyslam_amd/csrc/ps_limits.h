// ps_limits.h -- sizes that a kernel's layout fixes and that the option table (ps_options.h) bounds a user's value by.
// Plain preprocessor constants: included by ps_kernels.h, ahead of the kernel headers that use them (ps_k_xcg.h, ps_k_ldi.h),
// and by the host-only ps_options.h.
#pragma once

#define PS_XCG_MAXNODES 1024                  // coarse nodes of the explicit form (t of the big coarse kernel in LDS: 48 KB)
#define PS_LDI_MAXN 3328                      // unknowns of the lagged dense inverse (a row of X_u in 13 float4 per lane: PS_LDI_NF4)
