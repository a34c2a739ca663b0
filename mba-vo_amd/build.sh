#!/bin/bash
# Builds libmbavo.so (HIP kernels + host code + C ABI) for gfx950, in-tree.
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-result"
mkdir -p build
pids=()
for f in csrc/engine.hip csrc/ba_tracker.hip csrc/image_ops.hip csrc/keyframe_ops.hip csrc/lm_batch.hip csrc/pairs_prep.hip csrc/pairs_track.hip csrc/pairs_report.hip csrc/pairs_hyp.hip csrc/pairs_refine.hip csrc/pairs_filter.hip csrc/pairs_search.hip csrc/pairs_smooth.hip csrc/pairs_carry.hip csrc/pairs_prune.hip csrc/pairs_photo.hip csrc/pairs_photocal.hip csrc/pairs_score.hip csrc/multi_gpu.hip csrc/p2p_comm.hip; do
  o=build/$(basename "$f").o
  if [ ! -f "$o" ] || [ -n "$(find csrc -newer "$o" -print -quit)" ] || [ ../include/mbavo.h -nt "$o" ]; then
    # engine.hip without the SLP vectorizer: it packs the fp32 bilinear blend into v_pk_mul/add_f32 and then needs
    # more v_mov_b32 to arrange the pairs than it saves (sample loop 326 -> 318 VALU instructions, k_fused -1.5 us A/B)
    extra=""; [ "$f" = csrc/engine.hip ] && extra="-fno-slp-vectorize"
    $HIPCC $FLAGS $extra -c "$f" -o "$o" & pids+=($!)
  fi
done
for f in csrc/host_math.cpp csrc/tracker.cpp csrc/vo_frontend.cpp csrc/c_api.cpp; do
  o=build/$(basename "$f").o
  if [ ! -f "$o" ] || [ -n "$(find csrc -newer "$o" -print -quit)" ] || [ ../include/mbavo.h -nt "$o" ]; then
    $HIPCC $FLAGS -x hip -c "$f" -o "$o" & pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait "$p"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o libmbavo.so build/*.o -ldl
echo "built $(pwd)/libmbavo.so"
