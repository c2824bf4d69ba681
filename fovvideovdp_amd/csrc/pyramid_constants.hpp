// The strip geometry of the pyramid kernels (band_kernel.hpp, band2_kernel.hpp) that the host's launch plans (pyramid_host.hpp)
// share with them.  Plain constants: device and host code include it alike.
#pragma once

constexpr int STRIP_J = 60;     // coarse columns produced per wave (64 lanes - 2 halo lanes each side)

constexpr int F2_PITCH = 54;    // level-B columns owned per wave: lanes 6..59, all the two-level halo leaves valid (the kernel is
                                // co-bound -- its arithmetic alone takes as long as its data flow, profiles/r03_pyramid_bounds.md: 54 vs a line-aligned 52 columns measured +3.4 %)
constexpr int F2_HL = 6;        // halo lanes on the left (4 on the right); even, so lane parity == column parity
