#!/bin/bash
# row-class kernel durations against the resident waves per CU the grids are sized for (variant builds with
# -DSBX_PERMUTE_ROW_WAVES=<waves>, loaded through SBX_PROBE_LIB)
for wv in 4 8 12 16 24 32; do
  python3 tools/build_variant.py rw$wv sbx_permute.hip -DSBX_PERMUTE_ROW_WAVES=$wv > /dev/null || exit 1
  SBX_PROBE_LIB=rw$wv KT_N=40 tools/kt_permute.sh rw$wv "$@" > /dev/null
  echo "== waves/CU $wv"; grep -E "k_rows_quad" gpurun_out/kt_rw$wv.txt | head -5
done
