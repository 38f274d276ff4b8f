#!/bin/bash
# VGPR / SGPR / scratch of every render kernel variant and static instruction counts of the headline one (dev tool, no GPU needed)
# usage: tools/kernel_resources.sh [extra -D flags]
#        tools/kernel_resources.sh -DTERRA_RAY_SOURCE=1 [-DTERRA_RAY_HOLD=1]   the ray-sourced instances (the ray re-fetched per sample / held across a job)
#        tools/kernel_resources.sh -DTERRA_RAY_SOURCE=2                        the lens instances (include/terra_amd.h "Lens rendering")
#        tools/kernel_resources.sh -DTERRA_RAY_SOURCE=3 [-DTERRA_POINT_HOLD=1] the point instances (include/terra_amd.h "Point rendering": the point re-fetched per sample / held across a job)
#        tools/kernel_resources.sh --unit bake_kernels                          every kernel of another unit (terra_amd/csrc/<unit>.hip: bake_kernels, probe_kernels, ...), demangled
set -e
D=/tmp/terra_isa; rm -rf $D; mkdir -p $D; cd $D
if [ "$1" = "--unit" ]; then
    U=$2; shift 2
    /opt/rocm/bin/hipcc -x hip --offload-arch=gfx950 -std=c++17 -O3 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -fno-gpu-rdc -fno-slp-vectorize -I$OLDPWD/include "$@" --save-temps -c $OLDPWD/terra_amd/csrc/$U.hip -o u.o 2>/dev/null
    grep -E "^\s+\.(name|vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size):" $U-hip-amdgcn-amd-amdhsa-gfx950.s | paste - - - - - | sed -E 's/\s+/ /g' | awk '{print $4, "lds", $2, "priv", $6, "sgpr", $8, "vgpr", $10}' | c++filt | sed -E 's/\(anonymous namespace\):://; s/\(.*\) / /' | sort
    exit 0
fi
/opt/rocm/bin/hipcc -x hip --offload-arch=gfx950 -std=c++17 -O3 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -fno-gpu-rdc -fno-slp-vectorize -I$OLDPWD/include "$@" --save-temps -c $OLDPWD/terra_amd/csrc/render_kernels.hip -o rk.o 2>/dev/null
S=render_kernels-hip-amdgcn-amd-amdhsa-gfx950.s
grep -E "^\s+\.(name|vgpr_count|sgpr_count|private_segment_fixed_size):" $S | paste - - - - | sed -E 's/\s+/ /g' | grep terra_render_kernel | awk '{print $2, "priv", $4, "sgpr", $6, "vgpr", $8}' | sed 's/_Z19terra_render_kernelILi//; s/EEv15DevRenderParams//; s/EEv18DevRayRenderParams//; s/EEv19DevLensRenderParams//; s/EEv20DevPointRenderParams//; s/ELi/,/g' | sort | awk '{printf "<I,COUNT,MODE,KINDS>=%-12s %s %s %s %s %s %s\n",$1,$2,$3,$4,$5,$6,$7}' | grep -E "=0,0,1,1 |=1,0,1,1 |=0,0,0,1 |=0,0,2,1 |=1,0,2,1 |=0,0,2,63 |=0,0,1,3 |=0,2,1,1 " 
