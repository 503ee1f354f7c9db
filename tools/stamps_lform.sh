#!/bin/bash
# The layer-wise form's few-rows chain kernel (eh_lform_tailchain_kernel) with phase stamps: a second library whose entry-point units (eh_api.o
# and the units split off it: eh_lform.o holds the stamped kernels, eh_api.o the diagnostic branch of lean_refresh) are built with -DEH_STAMPS, then tools/stamps_lform.py prints the segments.   usage (repo root): bash tools/stamps_lform.sh   (build here, run on the GPU box)
set -e
here=$(cd "$(dirname "$0")/.." && pwd)
src=$here/easyhybrid.jl_amd/csrc
make -C $src -j8 >/dev/null
mkdir -p $src/build_stamps
flags=$(make -s -C $src print-cxxflags)
stamped=$(make -s -C $src print-apiobj)
for b in $stamped; do /opt/rocm/bin/hipcc $flags -DEH_STAMPS "$@" -c $src/${b%.o}.hip -o $src/build_stamps/$b; done
objs=""
for o in $src/build/*.o; do
  b=$(basename $o)
  case " $stamped " in *" $b "*) objs="$objs $src/build_stamps/$b";; *) objs="$objs $o";; esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o $here/easyhybrid.jl_amd/libeasyhybrid_hip_stamps.so $objs -L/opt/rocm/lib -lhiprtc -ldl -Wl,-rpath,/opt/rocm/lib -Wl,-soname,libeasyhybrid_hip.so
echo built $here/easyhybrid.jl_amd/libeasyhybrid_hip_stamps.so
