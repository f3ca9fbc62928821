# Build a diagnostics library variant with extra compile flags on every source (A/B runs):
#   bash tools/build_variant.sh <name> "<flags>"  ->  zk-odst_amd/variants/libb2f_<name>.so
set -e
cd "$(dirname "$0")/../zk-odst_amd"
N=$1; F=$2
make -s -j8 BUILD=variants/build_$N DIAG_LIB=variants/libb2f_$N.so EXTRA="$F" variants/libb2f_$N.so
rm -rf variants/build_$N
echo built variants/libb2f_$N.so
