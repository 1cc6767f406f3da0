#!/bin/sh
# Writes the gfx950 device assembly of every object of libgssd_hip.so to OUTDIR/<file>.s, compiled with the flags that
# csrc/Makefile gives that file (its compile lines, read with `make -n -B`, with `-c` turned into `--cuda-device-only -S`).
# Run it at two commits and compare with
#   diff -r -I __hip_cuid_ DIR_A DIR_B
# (the __hip_cuid_<hash> symbol is a hash of the translation unit and changes with any source edit).
# usage: scripts/device_asm.sh OUTDIR [JOBS]
set -eu
OUT=$(mkdir -p "$1" && cd "$1" && pwd)
JOBS=${2:-8}
cd "$(dirname "$0")/../grouped-ssd-pytorch_amd/gssd/csrc"
make -n -B | grep -- ' -c [a-z0-9_]*\.hip -o [a-z0-9_]*\.o$' |
    sed -e "s| -c \([a-z0-9_]*\)\.hip -o [a-z0-9_]*\.o\$| --cuda-device-only -S \1.hip -o $OUT/\1.s|" |
    xargs -P "$JOBS" -I{} sh -c '{}'
echo "$(ls "$OUT"/*.s | wc -l) files in $OUT"
