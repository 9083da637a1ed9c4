# Build libldso_ba.so of a git revision from that revision's own ldso_amd/csrc (every source and
# its Makefile), optionally with extra compiler flags and patches applied first, for
# LDSO_BA_LIB / tools/ab_libs.py:
#   bash tools/build_ab_rev.sh NAME REV ["-DFLAG=1 ..."] [PATCH ...]  ->  abl/NAME/libldso_ba.so
# The recorded patches (tools/rejected/, tools/diag/) apply to the revision tools/rejected/README.md names.
set -e
cd "$(dirname "$0")/.."
name=$1; rev=$2; flags=${3:-}; shift 2; [ $# -gt 0 ] && shift
out=abl/$name/src
mkdir -p $out
git archive "$rev" ldso_amd/csrc include | tar -x -C $out
for p in "$@"; do patch -s -p1 -d $out < "$p"; done
base=$(sed -n 's/^HIPFLAGS ?= //p' $out/ldso_amd/csrc/Makefile)
make -s -j4 -C $out/ldso_amd/csrc ../lib/libldso_ba.so HIPFLAGS="$base $flags"
cp $out/ldso_amd/lib/libldso_ba.so abl/$name/libldso_ba.so
