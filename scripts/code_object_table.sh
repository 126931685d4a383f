#!/bin/sh
# The gfx950 device code of one object file as a table: every function symbol with its code size, then every kernel with its
# registers, scratch and LDS.  Two builds whose tables are equal launch the same kernel instantiations with the same code --
# the check a host-only refactor of a .hip file has to pass (profiles/sort_stages_code_object_vs_parent.txt).
# Usage: scripts/code_object_table.sh cudf_amd/csrc/gx_sort.o > table.txt
set -eu
LLVM="${ROCM_PATH:-/opt/rocm}/llvm/bin"
obj="$1"
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
"$LLVM/llvm-objcopy" -O binary --only-section=.hip_fatbin "$obj" "$tmp/fatbin"
"$LLVM/clang-offload-bundler" --type=o --unbundle --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$tmp/fatbin" --output="$tmp/co"
echo "# function symbols: size name"
"$LLVM/llvm-readelf" -sW "$tmp/co" | awk '$4 == "FUNC" { print $3, $8 }' | sort -k2
echo "# kernels: name sgpr vgpr agpr scratch lds"
"$LLVM/llvm-readelf" --notes "$tmp/co" | awk '
  /\.agpr_count:/ { agpr = $NF }
  /\.group_segment_fixed_size:/ { lds = $NF }
  /\.name:/ { name = $NF }
  /\.private_segment_fixed_size:/ { scratch = $NF }
  /\.sgpr_count:/ { sgpr = $NF }
  /\.vgpr_count:/ { vgpr = $NF }
  /\.wavefront_size:/ { print name, sgpr, vgpr, agpr, scratch, lds }' | sort
