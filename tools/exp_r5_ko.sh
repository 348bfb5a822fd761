#!/bin/bash
# Round 5: where does the bf16 x 3 stem kernel's time go?  Phase timeline of the dominant pair (32 32 | 64 64) in the XM
# form (build: tools/build_variants.py tl=-DCTG_STEM_TIMELINE).  The second half of the experiment -- knock-out builds and
# the limb-intermediate form 2 next to it -- went with those switches; profiles/r5_stem_timeline_knockout.txt has its result.
R=${GRAFT_REPO_ROOT:-$PWD}; O=$R/gpurun_out/r5_ko; mkdir -p $O
X=$R/cotengra_amd/lib/exp
for form in 1; do
  CTG_LIB=$X/libctg_tl.so CTG_TL_SHAPE=${CTG_TL_SHAPE:-32,32,64,64} CTG_STEM_FORM=$form timeout 200 python $R/tools/exp_stem_timeline.py > $O/timeline_form$form.txt 2>&1
  cat $O/timeline_form$form.txt | grep -v amdgpu.ids
done
