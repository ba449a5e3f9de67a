#!/bin/bash
# conv_dma_x3's wide form (ko 710 where its rule holds) against the narrow form (ko 720) on the forward's two
# 240- / 480-channel strided convs, bitwise check included, then the knock-outs of both forms (KO bits of
# conv_dma_x3: 1 no split, 2 no B-piece reads, 4 no loop DMAs, 16 no epilogue; CB_X3CFG's NT = 15: the wide form)
# usage (GPU box): bash tools/gpu/dmax3_wide.sh OUTDIR
out=${1:?usage: dmax3_wide.sh OUTDIR}; mkdir -p $out; export TMPDIR=/tmp
CB=tools/bin/convbench
for rep in 1 2 3; do
  CB_CHECK=1 CB_STRIDE=2 CB_NORES=1 timeout -k 10 120 $CB sp 30 32 56 56 64 240 20 720 710 >> $out/cb.txt 2>&1 || { echo "layer2 failed"; tail $out/cb.txt; exit 1; }
  CB_CHECK=1 CB_STRIDE=2 CB_NORES=1 timeout -k 10 120 $CB sp 30 16 28 28 128 480 20 720 710 >> $out/cb.txt 2>&1 || { echo "layer3 failed"; tail $out/cb.txt; exit 1; }
done
CB_X3CFG="2 5 2" CB_STRIDE=2 CB_NORES=1 timeout -k 10 120 $CB sp 30 32 56 56 64 240 20 7232 7233 7234 7236 7248 >> $out/cb.txt 2>&1 || { echo "narrow knock-outs failed"; tail $out/cb.txt; exit 1; }
CB_X3CFG="2 15 2" CB_STRIDE=2 CB_NORES=1 timeout -k 10 120 $CB sp 30 32 56 56 64 240 20 7200 7201 7202 7204 7216 >> $out/cb.txt 2>&1 || { echo "wide knock-outs failed"; tail $out/cb.txt; exit 1; }
CB_X3CFG="2 15 2" CB_STRIDE=2 CB_NORES=1 timeout -k 10 120 $CB sp 30 16 28 28 128 480 20 7200 7201 7202 7204 7216 >> $out/cb.txt 2>&1 || { echo "wide knock-outs (layer3) failed"; tail $out/cb.txt; exit 1; }
cat $out/cb.txt
