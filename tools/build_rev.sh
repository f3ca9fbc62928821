# Build the diagnostics library of another git revision as an A/B variant, without #ifdef
# variants in the product sources: the revision's csrc/, Makefile and include/ are exported to a
# scratch tree and built there with that revision's own Makefile.
#   bash tools/build_rev.sh <rev> <name> ["<extra hipcc flags>"]  ->  zk-odst_amd/variants/libb2f_<name>.so
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
REV=$1; N=$2; F=${3:-}
T=$(mktemp -d /tmp/b2f_rev.XXXXXX)
mkdir -p $T/zk-odst_amd/csrc $T/include $ROOT/zk-odst_amd/variants
for f in $(git -C $ROOT ls-tree --name-only $REV zk-odst_amd/csrc/) zk-odst_amd/Makefile include/b2f.h; do
  git -C $ROOT show $REV:$f > $T/$f
done
OUT=$ROOT/zk-odst_amd/variants/libb2f_$N.so
cd $T/zk-odst_amd
if grep -q '^DIAG_LIB' Makefile; then
  make -s -j8 DIAG_LIB=$OUT EXTRA="$F" $OUT
else
  # a revision whose Makefile cannot name its output: every source it has, with its flags
  H="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -fvisibility=hidden --offload-arch=gfx950 -DB2F_DIAG $F"
  for f in csrc/*.hip; do
    case $f in
      csrc/b2f_kernels.hip|csrc/b2f_fused.hip) O="-mllvm -amdgpu-atomic-optimizer-strategy=None";;
      *) O=;;
    esac
    $H $O -c -o $(basename $f .hip).o $f &
  done
  wait
  $H -shared -o $OUT *.o
fi
rm -rf $T
echo built zk-odst_amd/variants/libb2f_$N.so from $REV
