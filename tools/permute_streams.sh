#!/bin/bash
# Permute2D end to end under different assignments of the row classes to side streams (variant builds with
# -DSBX_PERMUTE_CLASS_STREAMS="<six digits>", loaded through SBX_PROBE_LIB)
for m in 000000 023456 002222 000022; do
  python3 tools/build_variant.py cs$m sbx_permute.hip "-DSBX_PERMUTE_CLASS_STREAMS=\"$m\"" > /dev/null || exit 1
done
for rep in 1 2 3; do for m in 000000 023456 002222 000022; do
  echo -n "streams=$m: "; SBX_PROBE_LIB=cs$m python tools/permute_time.py | tail -2 | tr '\n' ' '; echo
done; done
