#!/bin/bash
# sort stage of the permute, per kernel: everything / no sort (rows stream out unsorted) / sort only (columns arrive
# relabelled: the same keys, no gather issued) / neither — timing ablation.  usage: tools/kt_ablate.sh [--rcm]
# (each mode is a variant build, -DSBX_PERMUTE_ABLATE=<bits> -DSBX_PERMUTE_ROW_WAVES=${RW:-16}, loaded through SBX_PROBE_LIB)
PAT="k_permute_tile<|k_rows_quad|k_permute_block_rows<int, 4, (256|512|1024),"
for mode in "0:full" "2:nosort" "4p:sortonly" "6:neither"; do
  f=${mode%%:*}; tag=${mode##*:}; extra=""
  if [ "$f" = "4p" ]; then f=4; extra="--prerelabel"; fi
  python3 tools/build_variant.py ab_$tag sbx_permute.hip -DSBX_PERMUTE_ABLATE=$f -DSBX_PERMUTE_ROW_WAVES=${RW:-16} > /dev/null || exit 1
  echo "== $tag (SBX_PERMUTE_ABLATE=$f $extra)"
  SBX_PROBE_LIB=ab_$tag KT_N=40 tools/kt_permute.sh ab_$tag "$@" $extra | grep -E "$PAT" | head -8
done
