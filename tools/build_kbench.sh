#!/bin/bash
# Build tools/kbench (production kernels) and tools/kbench_stamps (-DNODE_STAMPS diagnostic build): the kernel files it
# launches, the geometry (dims.hip) and the error text (host_common.hip) -- no solver.
set -e
cd "$(dirname "$0")/.."
SRC="neural-ode-features_amd/csrc"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -Wno-unused-function"
UNITS="tools/kbench.hip $SRC/kernels_layout.hip $SRC/kernels_groupnorm.hip $SRC/kernels_step_control.hip $SRC/kernels_generic.hip $SRC/kernels_theta_finalize.hip $SRC/kernels_conv_direct.hip $SRC/kernels_conv_wino1d.hip $SRC/kernels_conv_wino2d.hip $SRC/kernels_conv_small.hip $SRC/conv_select.hip $SRC/kernels_wgrad.hip $SRC/kernels_tiny.hip $SRC/kernels_tiny_solve.hip $SRC/dims.hip $SRC/host_common.hip"
/opt/rocm/bin/hipcc $FLAGS $UNITS -o tools/kbench &
P1=$!
/opt/rocm/bin/hipcc $FLAGS -DNODE_STAMPS $UNITS -o tools/kbench_stamps &
P2=$!
wait $P1
wait $P2
ls -la tools/kbench tools/kbench_stamps
