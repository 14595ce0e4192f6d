"""Which kernel a GEMM call is routed to (csrc/gemm_route.h), pinned on a machine without a GPU.

tests/gemm_route_dump.cpp -- a stand-alone program that includes only the route header -- prints the
route of a table of problems at 256 CUs: the step's shapes of tools/gemm_ab.py (NRMS and BERT
projection forward, dgrad and wgrad, the CNN tap projection, table dgrad and conv wgrad) in bf16x6 and
bf16, the shapes the GEMM GPU tests name (N = 1152 / 520 / 768 / 1100 / 1200, K = 480 / 544 / 992, with
and without a device-resident M), and one problem per remaining decision (under 400 tiles, unaligned,
CONV3 tap rules, the stream-K tail and the split-K slab with and without a workspace, the folded bias
gradient).  It is built here with g++ under the address and undefined-behaviour sanitizers and run as
a child process; its lines must equal EXPECTED.

EXPECTED records what the dispatch did BEFORE the route became a function: the lines were printed by
the previous nr_gemm_fast / gemm_static / gemm_dyn decision code, compiled verbatim with its kernel
launches replaced by recording stubs, over this same table.  A changed heuristic must change this
table in the same commit -- and then the GEMM GPU tests' docstrings say which kernel they mean.

modes: 0 KC_PLAIN, 1 KC_GATHER, 2 KC_CONV3, 3 MN_PLAIN, 4 MN_GATHER, 5 MN_CONV3 (A, B); tr: transposed
accumulators; epi: the epilogue the kernel runs (enum nr_epilogue)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gemm_route_dump.cpp")

EXPECTED = """\
nrms_proj_fwd bf16x6: big tile=256x256 planes=3 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
nrms_proj_fwd bf16: big tile=256x256 planes=1 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
nrms_proj_fwd_bound bf16x6: big tile=256x256 planes=3 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
nrms_proj_fwd_bound bf16: big tile=256x256 planes=1 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
nrms_proj_dgrad bf16x6: split_128 tile=128x128 planes=3 modes=0,3 tr=1 epi=0 splits=1 kchunk=1152 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
nrms_proj_dgrad bf16: split_128 tile=128x128 planes=1 modes=0,3 tr=1 epi=0 splits=1 kchunk=1152 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
nrms_dgrad_table bf16x6: big tile=256x256 planes=3 modes=0,3 tr=1 epi=7 splits=1 kchunk=1152 slab=0 fold=0 tail=16 tail_ws=0 tail_cap=0
nrms_dgrad_table bf16: big tile=256x256 planes=1 modes=0,3 tr=1 epi=7 splits=1 kchunk=1152 slab=0 fold=0 tail=16 tail_ws=0 tail_cap=0
nrms_dgrad_table_ws bf16x6: big tile=256x256 planes=3 modes=0,3 tr=1 epi=7 splits=1 kchunk=1152 slab=0 fold=0 tail=16 tail_ws=1 tail_cap=260
nrms_dgrad_table_ws bf16: big tile=256x256 planes=1 modes=0,3 tr=1 epi=7 splits=1 kchunk=1152 slab=0 fold=0 tail=16 tail_ws=0 tail_cap=0
nrms_dgrad_table_kc_ws bf16x6: big tile=256x256 planes=3 modes=0,0 tr=1 epi=7 splits=1 kchunk=1152 slab=0 fold=0 tail=16 tail_ws=1 tail_cap=260
nrms_dgrad_table_kc_ws bf16: big tile=256x256 planes=1 modes=0,0 tr=1 epi=7 splits=1 kchunk=1152 slab=0 fold=0 tail=16 tail_ws=0 tail_cap=0
nrms_dgrad_table_store bf16x6: split_128 tile=128x128 planes=3 modes=0,3 tr=1 epi=7 splits=1 kchunk=1152 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
nrms_dgrad_table_store bf16: split_128 tile=128x128 planes=1 modes=0,3 tr=1 epi=7 splits=1 kchunk=1152 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
nrms_proj_wgrad bf16x6: big tile=256x256 planes=3 modes=3,4 tr=0 epi=2 splits=17 kchunk=1472 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
nrms_proj_wgrad bf16: big tile=256x256 planes=1 modes=3,4 tr=0 epi=2 splits=17 kchunk=1472 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
nrms_proj_wgrad_ws bf16x6: big tile=256x256 planes=3 modes=3,4 tr=0 epi=2 splits=17 kchunk=1472 slab=1 fold=0 tail=0 tail_ws=0 tail_cap=0
nrms_proj_wgrad_ws bf16: big tile=256x256 planes=1 modes=3,4 tr=0 epi=2 splits=17 kchunk=1472 slab=1 fold=0 tail=0 tail_ws=0 tail_cap=0
nrms_proj_wgrad_cus bf16x6: big tile=256x256 planes=3 modes=3,4 tr=0 epi=2 splits=12 kchunk=2048 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
nrms_proj_wgrad_cus bf16: big tile=256x256 planes=1 modes=3,4 tr=0 epi=2 splits=12 kchunk=2048 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
bert_qkv bf16x6: big tile=256x256 planes=3 modes=0,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
bert_qkv bf16: big tile=256x256 planes=1 modes=0,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
bert_ffn1_gelu bf16x6: big tile=256x256 planes=3 modes=0,0 tr=1 epi=8 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
bert_ffn1_gelu bf16: big tile=256x256 planes=1 modes=0,0 tr=1 epi=8 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
bert_ffn2 bf16x6: big tile=256x256 planes=3 modes=0,0 tr=1 epi=0 splits=1 kchunk=3072 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
bert_ffn2 bf16: big tile=256x256 planes=1 modes=0,0 tr=1 epi=0 splits=1 kchunk=3072 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
bert_ffn2_dgrad bf16x6: big tile=256x256 planes=3 modes=0,3 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
bert_ffn2_dgrad bf16: big tile=256x256 planes=1 modes=0,3 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
bert_qkv_dgrad bf16x6: big tile=256x256 planes=3 modes=0,3 tr=1 epi=0 splits=1 kchunk=2304 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
bert_qkv_dgrad bf16: big tile=256x256 planes=1 modes=0,3 tr=1 epi=0 splits=1 kchunk=2304 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
bert_ffn1_wgrad bf16x6: big tile=256x256 planes=3 modes=3,3 tr=0 epi=2 splits=7 kchunk=2976 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
bert_ffn1_wgrad bf16: big tile=256x256 planes=1 modes=3,3 tr=0 epi=2 splits=7 kchunk=2976 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
bert_ffn1_wgrad_cs bf16x6: big tile=256x256 planes=3 modes=3,3 tr=0 epi=2 splits=7 kchunk=2976 slab=1 fold=1 tail=0 tail_ws=0 tail_cap=0
bert_ffn1_wgrad_cs bf16: big tile=256x256 planes=1 modes=3,3 tr=0 epi=2 splits=7 kchunk=2976 slab=1 fold=1 tail=0 tail_ws=0 tail_cap=0
bert_ffn2_wgrad_cs bf16x6: big tile=256x256 planes=3 modes=3,3 tr=0 epi=2 splits=7 kchunk=2976 slab=1 fold=1 tail=0 tail_ws=0 tail_cap=0
bert_ffn2_wgrad_cs bf16: big tile=256x256 planes=1 modes=3,3 tr=0 epi=2 splits=7 kchunk=2976 slab=1 fold=1 tail=0 tail_ws=0 tail_cap=0
bert_qkv_wgrad_cs bf16x6: big tile=256x256 planes=3 modes=3,3 tr=0 epi=2 splits=9 kchunk=2336 slab=1 fold=1 tail=0 tail_ws=0 tail_cap=0
bert_qkv_wgrad_cs bf16: big tile=256x256 planes=1 modes=3,3 tr=0 epi=2 splits=9 kchunk=2336 slab=1 fold=1 tail=0 tail_ws=0 tail_cap=0
cnn_tap_proj bf16x6: big tile=256x256 planes=3 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
cnn_tap_proj bf16: big tile=256x256 planes=1 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
cnn_tap_proj_mdev bf16x6: big tile=256x256 planes=3 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
cnn_tap_proj_mdev bf16: big tile=256x256 planes=1 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
cnn_table_dgrad bf16x6: split_128 tile=128x128 planes=3 modes=0,3 tr=1 epi=7 splits=1 kchunk=480 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
cnn_table_dgrad bf16: split_128 tile=128x128 planes=1 modes=0,3 tr=1 epi=7 splits=1 kchunk=480 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
cnn_table_dgrad_kc bf16x6: split_128 tile=128x128 planes=3 modes=0,0 tr=1 epi=7 splits=1 kchunk=480 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
cnn_table_dgrad_kc bf16: split_128 tile=128x128 planes=1 modes=0,0 tr=1 epi=7 splits=1 kchunk=480 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
cnn_table_dgrad_ws bf16x6: big tile=256x256 planes=3 modes=0,3 tr=1 epi=7 splits=1 kchunk=480 slab=0 fold=0 tail=16 tail_ws=1 tail_cap=260
cnn_table_dgrad_ws bf16: split_128 tile=128x128 planes=1 modes=0,3 tr=1 epi=7 splits=1 kchunk=480 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
cnn_conv_wgrad bf16x6: big tile=256x256 planes=3 modes=3,4 tr=0 epi=2 splits=41 kchunk=608 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
cnn_conv_wgrad bf16: big tile=256x256 planes=1 modes=3,4 tr=0 epi=2 splits=41 kchunk=608 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
cnn_conv_wgrad_ws bf16x6: big tile=256x256 planes=3 modes=3,4 tr=0 epi=2 splits=41 kchunk=608 slab=1 fold=0 tail=0 tail_ws=0 tail_cap=0
cnn_conv_wgrad_ws bf16: big tile=256x256 planes=1 modes=3,4 tr=0 epi=2 splits=41 kchunk=608 slab=1 fold=0 tail=0 tail_ws=0 tail_cap=0
user_fwd bf16x6: f32_64 tile=64x64 planes=0 modes=0,0 tr=1 epi=0 splits=1 kchunk=384 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
user_fwd bf16: split_128 tile=128x128 planes=1 modes=0,0 tr=1 epi=0 splits=1 kchunk=384 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
user_wgrad_cs bf16x6: f32_64 tile=64x64 planes=0 modes=3,3 tr=0 epi=2 splits=3 kchunk=544 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
user_wgrad_cs bf16: big tile=256x128 planes=1 modes=3,3 tr=0 epi=2 splits=3 kchunk=544 slab=1 fold=1 tail=0 tail_ws=0 tail_cap=0
test_split_plain_kk bf16x6: split_128 tile=128x128 planes=3 modes=0,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_split_plain_kk bf16: split_128 tile=128x128 planes=1 modes=0,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_split_plain_km bf16x6: split_128 tile=128x128 planes=3 modes=0,3 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_split_plain_km bf16: split_128 tile=128x128 planes=1 modes=0,3 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_split_plain_mm bf16x6: big tile=256x128 planes=3 modes=3,3 tr=0 epi=2 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_split_plain_mm bf16: big tile=256x128 planes=1 modes=3,3 tr=0 epi=2 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_split_plain_static bf16x6: f32_64 tile=64x64 planes=0 modes=0,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_split_plain_static bf16: split_128 tile=128x128 planes=1 modes=0,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_gather_n1152 bf16x6: split_128 tile=128x128 planes=3 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_gather_n1152 bf16: split_128 tile=128x128 planes=1 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_big_n1100 bf16x6: split_128 tile=128x128 planes=3 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_big_n1100 bf16: split_128 tile=128x128 planes=1 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_big_n1100_mdev bf16x6: big tile=256x256 planes=3 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_big_n1100_mdev bf16: big tile=256x256 planes=1 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_big_n1200 bf16x6: split_128 tile=128x128 planes=3 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_big_n1200 bf16: split_128 tile=128x128 planes=1 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_big_n768_mdev bf16x6: big tile=256x256 planes=3 modes=0,3 tr=1 epi=7 splits=1 kchunk=1152 slab=0 fold=0 tail=16 tail_ws=0 tail_cap=0
test_big_n768_mdev bf16: big tile=256x256 planes=1 modes=0,3 tr=1 epi=7 splits=1 kchunk=1152 slab=0 fold=0 tail=16 tail_ws=0 tail_cap=0
test_k480 bf16x6: split_128 tile=128x128 planes=3 modes=0,3 tr=1 epi=7 splits=1 kchunk=480 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_k480 bf16: split_128 tile=128x128 planes=1 modes=0,3 tr=1 epi=7 splits=1 kchunk=480 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_k544 bf16x6: big tile=256x256 planes=3 modes=0,3 tr=1 epi=7 splits=1 kchunk=544 slab=0 fold=0 tail=16 tail_ws=0 tail_cap=0
test_k544 bf16: big tile=256x256 planes=1 modes=0,3 tr=1 epi=7 splits=1 kchunk=544 slab=0 fold=0 tail=16 tail_ws=0 tail_cap=0
test_k544_ws bf16x6: big tile=256x256 planes=3 modes=0,3 tr=1 epi=7 splits=1 kchunk=544 slab=0 fold=0 tail=16 tail_ws=1 tail_cap=260
test_k544_ws bf16: big tile=256x256 planes=1 modes=0,3 tr=1 epi=7 splits=1 kchunk=544 slab=0 fold=0 tail=16 tail_ws=0 tail_cap=0
test_k992_wgrad bf16x6: big tile=256x256 planes=3 modes=3,4 tr=0 epi=2 splits=1 kchunk=992 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_k992_wgrad bf16: big tile=256x256 planes=1 modes=3,4 tr=0 epi=2 splits=1 kchunk=992 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_k992_wgrad_ws bf16x6: big tile=256x256 planes=3 modes=3,4 tr=0 epi=2 splits=1 kchunk=992 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
test_k992_wgrad_ws bf16: big tile=256x256 planes=1 modes=3,4 tr=0 epi=2 splits=1 kchunk=992 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
small_static bf16x6: f32_64 tile=64x64 planes=0 modes=0,0 tr=1 epi=0 splits=1 kchunk=96 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
small_static bf16: split_128 tile=128x128 planes=1 modes=0,0 tr=1 epi=0 splits=1 kchunk=96 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
small_dyn bf16x6: split_128 tile=128x128 planes=3 modes=0,0 tr=1 epi=0 splits=1 kchunk=96 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
small_dyn bf16: split_128 tile=128x128 planes=1 modes=0,0 tr=1 epi=0 splits=1 kchunk=96 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
unaligned_static bf16x6: generic tile=64x64 planes=0 modes=0,0 tr=0 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
unaligned_static bf16: generic tile=64x64 planes=0 modes=0,0 tr=0 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
unaligned_dyn bf16x6: not_eligible einval=7
unaligned_dyn bf16: not_eligible einval=7
odd_ld_static bf16x6: generic tile=64x64 planes=0 modes=0,0 tr=0 epi=0 splits=1 kchunk=96 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
odd_ld_static bf16: generic tile=64x64 planes=0 modes=0,0 tr=0 epi=0 splits=1 kchunk=96 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
k_zero_static bf16x6: generic tile=64x64 planes=0 modes=0,0 tr=0 epi=0 splits=1 kchunk=32 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
k_zero_static bf16: generic tile=64x64 planes=0 modes=0,0 tr=0 epi=0 splits=1 kchunk=32 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
conv3_fwd bf16x6: split_128 tile=128x128 planes=3 modes=2,0 tr=1 epi=1 splits=1 kchunk=2304 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
conv3_fwd bf16: split_128 tile=128x128 planes=1 modes=2,0 tr=1 epi=1 splits=1 kchunk=2304 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
conv3_wgrad bf16x6: split_128 tile=128x128 planes=3 modes=3,5 tr=0 epi=2 splits=8 kchunk=3008 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
conv3_wgrad bf16: split_128 tile=128x128 planes=1 modes=3,5 tr=0 epi=2 splits=8 kchunk=3008 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
conv3_wgrad_seg_96 bf16x6: not_eligible einval=7
conv3_wgrad_seg_96 bf16: not_eligible einval=7
conv3_kc_seg_20 bf16x6: not_eligible einval=6
conv3_kc_seg_20 bf16: not_eligible einval=6
conv3_mn_seg_20 bf16x6: not_eligible einval=7
conv3_mn_seg_20 bf16: not_eligible einval=7
zeroed_small_ws bf16x6: big tile=256x256 planes=3 modes=0,3 tr=1 epi=7 splits=1 kchunk=1152 slab=0 fold=0 tail=16 tail_ws=0 tail_cap=0
zeroed_small_ws bf16: big tile=256x256 planes=1 modes=0,3 tr=1 epi=7 splits=1 kchunk=1152 slab=0 fold=0 tail=16 tail_ws=0 tail_cap=0
splitk_small_ws bf16x6: big tile=256x256 planes=3 modes=3,3 tr=0 epi=2 splits=17 kchunk=1472 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
splitk_small_ws bf16: big tile=256x256 planes=1 modes=3,3 tr=0 epi=2 splits=17 kchunk=1472 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
splitk_atomic bf16x6: big tile=256x256 planes=3 modes=3,3 tr=0 epi=2 splits=17 kchunk=1472 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
splitk_atomic bf16: big tile=256x256 planes=1 modes=3,3 tr=0 epi=2 splits=17 kchunk=1472 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
splitk_slab bf16x6: big tile=256x256 planes=3 modes=3,3 tr=0 epi=2 splits=17 kchunk=1472 slab=1 fold=0 tail=0 tail_ws=0 tail_cap=0
splitk_slab bf16: big tile=256x256 planes=1 modes=3,3 tr=0 epi=2 splits=17 kchunk=1472 slab=1 fold=0 tail=0 tail_ws=0 tail_cap=0
splitk_slab_fold bf16x6: big tile=256x256 planes=3 modes=3,3 tr=0 epi=2 splits=17 kchunk=1472 slab=1 fold=1 tail=0 tail_ws=0 tail_cap=0
splitk_slab_fold bf16: big tile=256x256 planes=1 modes=3,3 tr=0 epi=2 splits=17 kchunk=1472 slab=1 fold=1 tail=0 tail_ws=0 tail_cap=0
splitk_slab_gather_colsum bf16x6: big tile=256x256 planes=3 modes=3,4 tr=0 epi=2 splits=17 kchunk=1472 slab=1 fold=1 tail=0 tail_ws=0 tail_cap=0
splitk_slab_gather_colsum bf16: big tile=256x256 planes=1 modes=3,4 tr=0 epi=2 splits=17 kchunk=1472 slab=1 fold=1 tail=0 tail_ws=0 tail_cap=0
splitk_scatter bf16x6: split_128 tile=128x128 planes=3 modes=0,3 tr=0 epi=3 splits=4 kchunk=576 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
splitk_scatter bf16: split_128 tile=128x128 planes=1 modes=0,3 tr=0 epi=3 splits=4 kchunk=576 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
bert_qkv f32: f32_128 tile=128x128 planes=0 modes=0,0 tr=1 epi=0 splits=1 kchunk=768 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
small_static f32: f32_64 tile=64x64 planes=0 modes=0,0 tr=1 epi=0 splits=1 kchunk=96 slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0
"""


@pytest.fixture(scope="module")
def route_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/gemm_route_dump.cpp"
    exe = str(tmp_path_factory.mktemp("route") / "gemm_route_dump")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True, capture_output=True, text=True)
    return exe


def _lines(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == ""   # no sanitizer report
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def dumped(route_exe):
    return _lines(route_exe)


def test_k_split_rule(route_exe):
    """k_chunk / k_split (gemm_route.h), the one K-split rule of the host and the kernels, over
    K in {32, 64, 96, 480, 1152, 20832} x want in 1..64: k_chunk is ceil32(ceil(K / want)) (32 when
    that is 0); k_split takes that chunk and counts the splits that hold some of K; and the chunk the
    kernels recompute from the route's split count (clamp_extents, splitk_reduce_kernel) is the
    route's own chunk."""
    rows = [tuple(int(x) for x in l.split()) for l in _lines(route_exe, "ksplit")]
    assert [(k, w) for k, w, *_ in rows] == [(k, w) for k in (32, 64, 96, 480, 1152, 20832) for w in range(1, 65)]
    for K, want, chunk, ks_chunk, ks_splits, chunk_of_splits in rows:
        formula = -(-(-(-K // want)) // 32) * 32 or 32
        assert chunk == formula, (K, want)
        assert ks_chunk == chunk, (K, want)
        assert ks_splits == -(-K // ks_chunk), (K, want)
        assert chunk_of_splits == ks_chunk, (K, want, ks_splits)


def test_walk_cases_route_where_they_say(route_exe):
    """The multi-unit cases of tests/test_gemm_walk_gpu.py land on the kernel family, tile, planes,
    operand modes and split count their table names (tests/gemm_walk_util.py)."""
    import gemm_epi_util as U
    import gemm_walk_util as W
    for case in W.ALL_CASES:
        lines = _lines(route_exe, *W.route_argv(case))
        assert len(lines) == 1
        got, want = U.parse_route(lines[0]), W.route_fields(case)
        assert {f: got.get(f) for f in want} == want, (case.id, got)


def test_routes_match_the_recorded_table(dumped):
    want = EXPECTED.splitlines()
    assert len(dumped) == len(want)
    for got, exp in zip(dumped, want):
        assert got == exp


def test_nrms_projection_forward_anchor(dumped):
    """M = 23872, N = 1152, K = 768, gathered K-contiguous A, plain K-contiguous B, bf16x6, m_dev, EPI_STORE:
    by hand -- K >= 512, 94 row tiles >= 8, and a device-resident M with N >= 1024 takes the 256 x 256 tiles
    (the round efficiencies agree: 470 units in 2 rounds of 256 x 0.9 useful columns = 0.826 against
    0.87 x 0.822 for 1683 units in 4 rounds of 512); one split -- and in the recorded step trace:
    gemm_big_kernel<1, 0, true, 3, 256>."""
    line = [l for l in dumped if l.startswith("nrms_proj_fwd bf16x6:")]
    assert line == ["nrms_proj_fwd bf16x6: big tile=256x256 planes=3 modes=1,0 tr=1 epi=0 splits=1 kchunk=768 "
                    "slab=0 fold=0 tail=0 tail_ws=0 tail_cap=0"]


def test_every_family_is_in_the_table(dumped):
    seen = {l.split(": ")[1].split(" ")[0] for l in dumped}
    assert seen == {"not_eligible", "generic", "f32_64", "f32_128", "split_128", "big"}
