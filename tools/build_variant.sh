# Build lightzero_amd/liblzm_var<NAME>.so from the sources of git revision REV (default: the working tree),
# for interleaved A/B runs (tools/ab_libs.sh). usage: bash tools/build_variant.sh NAME [REV] [extra hipcc flags]
# Builds what lightzero_amd/build.py builds: lzm_kernels.hip, and, where the revision has them, lzm_az_c4.hip, lzm_az_gomoku.hip,
# lzm_az_gomoku_n.hip, lzm_az_gomoku_n_split.hip, lzm_search_stoch_mlp.hip, lzm_search_sampled_mlp.hip and lzm_smz_conv.hip as units of their own with the packed-f32 VALU forms
# switched off.
set -e
name=$1; rev=${2:-}; shift; shift || true
root=$(cd "$(dirname "$0")/.." && pwd)
src=$root
if [ -n "$rev" ]; then
  src=$(mktemp -d /tmp/lzm_var_XXXX)
  git -C "$root" archive "$rev" lightzero_amd/csrc include | tar -x -C "$src"
fi
flags="-O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC -Wall --offload-arch=gfx950"
objs=
tmp=$(mktemp -d /tmp/lzm_var_obj_XXXX)
for unit in lzm_az_c4 lzm_az_gomoku lzm_az_gomoku_n lzm_az_gomoku_n_split lzm_search_stoch_mlp lzm_search_sampled_mlp lzm_smz_conv; do
  if [ -f "$src/lightzero_amd/csrc/$unit.hip" ]; then
    /opt/rocm/bin/hipcc $flags "$@" -Xclang -target-feature -Xclang -packed-fp32-ops -c -o "$tmp/$unit.o" \
      "$src/lightzero_amd/csrc/$unit.hip"
    objs="$objs $tmp/$unit.o"
  fi
done
/opt/rocm/bin/hipcc $flags -shared "$@" -o "$root/lightzero_amd/liblzm_var$name.so" $objs \
  "$src/lightzero_amd/csrc/lzm_kernels.hip"
echo "built lightzero_amd/liblzm_var$name.so from ${rev:-working tree}"
