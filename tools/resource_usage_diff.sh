# Per-kernel resource lines (-Rpass-analysis=kernel-resource-usage) of lzm_kernels.hip at git revision REV against
# the working tree's, as a diff, then the lines of the Connect4 unit (lzm_az_c4.hip), which REV may not have.
# Source line numbers are stripped so that moved code does not show. Two full compiles, side by side.
# usage: bash tools/resource_usage_diff.sh REV > profiles/az_connect4/resource_usage.diff
set -e
rev=$1
root=$(cd "$(dirname "$0")/.." && pwd)
old=$(mktemp -d /tmp/lzm_res_XXXX)
git -C "$root" archive "$rev" lightzero_amd/csrc include | tar -x -C "$old"
flags="-O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC -Wall --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage"
lines() {  # $1: source file, $2..: extra flags -> normalised remark lines
  src=$1; shift
  /opt/rocm/bin/hipcc $flags "$@" -c -o /dev/null "$src" 2>&1 | grep "remark:" |
    sed -E 's#^(remark: )?[^ ]*/csrc/##; s#^([A-Za-z_0-9.]+):[0-9]+:[0-9]+: (remark: )?#\1: #; s# \[-Rpass-analysis=kernel-resource-usage\]##'
}
lines "$old/lightzero_amd/csrc/lzm_kernels.hip" > "$old/parent.txt" &
lines "$root/lightzero_amd/csrc/lzm_kernels.hip" > "$old/tree.txt"
wait
echo "# $(basename "$0") $rev: lzm_kernels.hip, $(grep -c 'Function Name' "$old/parent.txt") kernels in $rev," \
     "$(grep -c 'Function Name' "$old/tree.txt") in the working tree"
echo "# ---- diff parent tree (nothing between this line and the next marker: no line differs)"
diff "$old/parent.txt" "$old/tree.txt" || true
echo "# ---- lzm_az_c4.hip (working tree)"
lines "$root/lightzero_amd/csrc/lzm_az_c4.hip" -Xclang -target-feature -Xclang -packed-fp32-ops
echo "# ---- lzm_search_stoch_mlp.hip (working tree)"
lines "$root/lightzero_amd/csrc/lzm_search_stoch_mlp.hip" -Xclang -target-feature -Xclang -packed-fp32-ops
echo "# ---- lzm_search_sampled_mlp.hip (working tree)"
lines "$root/lightzero_amd/csrc/lzm_search_sampled_mlp.hip" -Xclang -target-feature -Xclang -packed-fp32-ops
echo "# ---- lzm_az_gomoku.hip (working tree)"
lines "$root/lightzero_amd/csrc/lzm_az_gomoku.hip" -Xclang -target-feature -Xclang -packed-fp32-ops
echo "# ---- lzm_az_gomoku_n.hip (working tree)"
lines "$root/lightzero_amd/csrc/lzm_az_gomoku_n.hip" -Xclang -target-feature -Xclang -packed-fp32-ops
echo "# ---- lzm_az_gomoku_n_split.hip (working tree)"
lines "$root/lightzero_amd/csrc/lzm_az_gomoku_n_split.hip" -Xclang -target-feature -Xclang -packed-fp32-ops
