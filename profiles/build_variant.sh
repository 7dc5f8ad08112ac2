#!/bin/bash
# A tuning variant of the library with only SOME translation units recompiled (the others come from the product's
# objects in diral_amd/build/): seconds instead of minutes.  Build container.
#   bash profiles/build_variant.sh <name> "<-D flags>" <tu> [tu ...]     ->  variants_tmp/lib_<name>.so
# e.g. bash profiles/build_variant.sh x1 "-DDIRAL_WIDE_BENCH_ONLY -DFOO=1" k_wide4
set -e
cd "$(dirname "$0")/.."
NAME=$1; FLAGS=$2; shift 2
mkdir -p variants_tmp/obj_$NAME
# the translation units, the compiler and its flags: the build's own (diral_amd/build.py)
eval "$(python3 -c 'from diral_amd import build as b; print("TUS=\"%s\"; CC=\"%s\"; CFLAGS=\"%s\"" % (" ".join(s[:-4] for s in b.SOURCES), b.hipcc_path(), " ".join(b.HIPCC_FLAGS)))')"
OBJS=""
for tu in $TUS; do
  if [[ " $* " == *" $tu "* ]]; then
    $CC $CFLAGS $FLAGS -c diral_amd/csrc/$tu.hip -o variants_tmp/obj_$NAME/$tu.o &
    OBJS="$OBJS variants_tmp/obj_$NAME/$tu.o"
  else
    OBJS="$OBJS diral_amd/build/$tu.o"
  fi
done
wait
$CC --offload-arch=gfx950 -shared -fPIC $OBJS -o variants_tmp/lib_$NAME.so
ls -la variants_tmp/lib_$NAME.so
