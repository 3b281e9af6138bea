# timing decomposition of the NCHW-direct decoded first layer (variants built by scripts/build_variant.sh _nv<bits> qcnn_decoded.hip
# -DNCHW_VAR=<bits>; results wrong, timing only).  The default run takes the two-piece fp16 kernel (QCNN_OPT_DEC_BF16SPLIT = 2): bits
# 1 no operand loads, 2 no products, 4 no stores, 8 no split and no range test, 32 no fix-up launch behind it (the guard's cost)
for v in ${VARIANTS:-"" _nv1 _nv2 _nv4 _nv8 _nv32}; do
QCNN_HIP_LIB=$PWD/quantized-cnn_amd/libqcnn_hip$v.so python bench.py --steps 6 --warmup 2 --extras 0 --cpu-sample 0 --parity-images 0 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.readline()); lm=d['roofline']['layer_ms']; print('variant [$v]', d['value'], 'conv1', lm.get('00_conv'))"
done
