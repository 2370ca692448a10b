"""-m gpu: the training attention kernels (attention.hip) per element against float64, under the bound of tests/attention_bounds.py.

Every case runs cmp_k_attn_fwd, then cmp_k_attn_bwd on the o and lse that forward stored, with the c_attn bias gradient armed, on
planted inputs (attention_bounds.attn_inputs: every query weights one partner key at ~0.4, the partner offsets cycling over the
(batch, head) groups through both sides of 32, 64, 128 and 256) at p = 0 and 0.2; operands and results live in a guard-banded Arena.
o, dq, dk, dv are held per element to  2 max(q2, u) S2 (+ 2^-8 |ref| in bf16),  lse and delta to  4 floor + 1e-6 max |ref|  in both
modes -- the bf16 lse is an fp32 quantity and is held as one.  tests/test_attention_checks_host.py shows on the CPU that these limits
reject a dropped key, a skipped sub-tile, a diagonal off by one and eleven other faults, and that on these inputs ANY single deleted
key moves o, dq, dk, dv and lse by at least ten limits; the old global-maximum metric passed a skipped 64-key tile.

What each table is for (tests/test_attn_plan_host.py holds every row to the launch form named here):
  TILE_EDGE       B 1, H 2, D 16 and 64, both dtypes, T = 1, 2 and both sides of 32, 64, 128, 256: every ragged sub-tile, tile and block edge.
                  bf16 at D = 16 runs the key-split set from T = 64 on (one launch), everything else the 128-row kernels.
  ROWS_333        the 128-row forward, dQ and dK/dV kernels with three query blocks, a ragged 64-key tile and a ragged 32-key sub-tile: fp32
                  and bf16 at D = 64 and 128; bf16 at D = 16 and 32 with 3 * 48 = 144 > 128 workgroups (past the key split); one row per
                  dtype with scale = 0 (scores unscaled).
  KEY_SPLIT_ONE   bf16, D = 16 and 32, 8 groups: forward key-split and the whole backward in ONE launch (2 * 11 * 8 = 176 <= 512 workgroups).
  KEY_SPLIT_TWO   the same with 32 groups: 3 * 32 = 96 <= 128, 22 * 32 = 704 > 512 -> dQ and dK/dV key-split launches apart.
  LN_ROWS         the rstd-scaled backward (cmp_attn_bwd_ln_next) on one row of test_gpu_ln_fused.ATTN_LN_ROWS_HEADS.
The long and planned shapes (paired blocks, block plans, long key-split rows) are the tables of tests/test_gpu_kernels.py, whose
check_attention_groups now also applies `attn_check`, on its randn inputs and on planted ones.  The masked forward
(CMP_ATTN_FWD_MASK) has no kernel-level entry point and stays with its model-level test (tests/test_gpu_model.py).

Limits.  bf16 mode: 2 max(q2, u) S2 + 2^-8 |ref| and nothing else.  fp32 mode adds the allowances of attention_bounds.f32_allowances
(4 x the emulation's deviation from float64 in the fp32 chains behind a score and behind dP - delta, relative to each chain's size, the
largest over the case): with q2 over the case alone, three fp32 cases of the 166 stood outside -- T = 1, D = 64, p = 0.2: dq and dk at 1.07;
T = 2, D = 64, p = 0.2: o at 1.003; T = 32, D = 16, p = 0.2: dq at 1.25 -- every other output of every case inside.  In those cases the
elements of a row share one draw of the chains' roundings (at T = 1 dq and dk ARE the residue of the dP and delta chains,
attention.hip:198 and :784-790), so q2 over two groups of one or two rows samples two to four draws.  The allowances make the fp32
limits 3 to 6 times the quadrature term; the CPU proofs (wrong kernels rejected, ten limits per deleted key) run under the same limits.
Two earlier findings were the emulation's and are in it with their kernel lines: the fp32 kernels accumulate every product as one
chain (:84, :198, :213), which numpy's blocked float32 product under-samples, and delta is summed as two interleaved half-rows
(:784-790) while dP is one chain.  No kernel was changed.  The rstd-scaled backward sums the c_attn bias gradient in front of the rstd
factor; its case checks the armed vector against the stored rows divided by their rstd.

Measured on an MI355X, every case: error / limit of o lse dq dk dv delta | q2 of o dq dk dv in units of u (2^-24 fp32, 2^-9 bf16), from the
CPU emulation over the checked groups.  Worst error / limit of all: o 0.66, lse 0.13, dq 0.72, dk 0.68, dv 0.68, delta 0.13 (fp32 cases: 0.40).
The last 44 lines are the tables of tests/test_gpu_kernels.py on randn and on planted inputs.
  fp32 B1 T1 H2 D16 scale1 p0.0          0.00 0.03 0.17 0.17 0.00 0.03 | 0.0 0.0 0.0 0.0
  fp32 B1 T1 H2 D16 scale1 p0.2          0.07 0.03 0.04 0.04 0.07 0.08 | 0.9 1.9 1.9 0.9
  fp32 B1 T2 H2 D16 scale1 p0.0          0.09 0.05 0.05 0.05 0.08 0.03 | 6.2 5.7 5.0 4.9
  fp32 B1 T2 H2 D16 scale1 p0.2          0.05 0.05 0.05 0.05 0.07 0.02 | 5.7 4.6 4.7 5.0
  fp32 B1 T31 H2 D16 scale1 p0.0         0.14 0.06 0.08 0.10 0.18 0.06 | 9.6 17.1 12.6 12.3
  fp32 B1 T31 H2 D16 scale1 p0.2         0.13 0.06 0.07 0.08 0.11 0.05 | 10.6 12.0 14.7 11.2
  fp32 B1 T32 H2 D16 scale1 p0.0         0.11 0.06 0.07 0.08 0.14 0.04 | 13.0 16.7 11.5 14.7
  fp32 B1 T32 H2 D16 scale1 p0.2         0.12 0.06 0.07 0.08 0.13 0.05 | 13.3 19.3 13.1 12.2
  fp32 B1 T33 H2 D16 scale1 p0.0         0.13 0.05 0.08 0.09 0.17 0.02 | 13.1 14.0 14.6 12.5
  fp32 B1 T33 H2 D16 scale1 p0.2         0.14 0.05 0.08 0.09 0.13 0.03 | 8.4 12.1 13.5 12.7
  fp32 B1 T63 H2 D16 scale1 p0.0         0.17 0.06 0.08 0.11 0.14 0.05 | 12.8 15.6 18.4 19.7
  fp32 B1 T63 H2 D16 scale1 p0.2         0.17 0.06 0.08 0.12 0.11 0.07 | 14.3 16.6 12.3 16.8
  fp32 B1 T64 H2 D16 scale1 p0.0         0.15 0.06 0.07 0.07 0.14 0.04 | 16.6 17.0 18.2 14.0
  fp32 B1 T64 H2 D16 scale1 p0.2         0.16 0.06 0.09 0.08 0.17 0.03 | 16.1 17.3 13.1 15.4
  fp32 B1 T65 H2 D16 scale1 p0.0         0.12 0.06 0.07 0.12 0.15 0.05 | 13.2 19.7 14.5 17.4
  fp32 B1 T65 H2 D16 scale1 p0.2         0.11 0.06 0.07 0.11 0.16 0.07 | 15.1 21.6 18.8 16.7
  fp32 B1 T127 H2 D16 scale1 p0.0        0.10 0.05 0.07 0.12 0.16 0.04 | 23.5 28.7 25.9 23.9
  fp32 B1 T127 H2 D16 scale1 p0.2        0.10 0.05 0.05 0.11 0.13 0.05 | 23.2 28.1 27.2 25.1
  fp32 B1 T128 H2 D16 scale1 p0.0        0.12 0.06 0.06 0.08 0.14 0.07 | 26.5 24.0 24.7 22.8
  fp32 B1 T128 H2 D16 scale1 p0.2        0.14 0.06 0.06 0.08 0.14 0.06 | 19.5 32.6 19.6 18.4
  fp32 B1 T129 H2 D16 scale1 p0.0        0.12 0.06 0.07 0.12 0.16 0.05 | 19.4 25.5 26.8 25.5
  fp32 B1 T129 H2 D16 scale1 p0.2        0.10 0.06 0.07 0.11 0.13 0.04 | 20.1 25.0 23.6 25.5
  fp32 B1 T255 H2 D16 scale1 p0.0        0.14 0.07 0.07 0.13 0.23 0.05 | 25.7 36.9 35.4 42.9
  fp32 B1 T255 H2 D16 scale1 p0.2        0.15 0.07 0.07 0.16 0.13 0.06 | 27.9 31.6 32.0 32.9
  fp32 B1 T256 H2 D16 scale1 p0.0        0.15 0.06 0.08 0.13 0.20 0.05 | 31.1 27.8 36.1 33.6
  fp32 B1 T256 H2 D16 scale1 p0.2        0.15 0.06 0.07 0.12 0.18 0.05 | 31.3 32.4 34.3 29.9
  fp32 B1 T257 H2 D16 scale1 p0.0        0.14 0.07 0.09 0.11 0.14 0.05 | 30.1 23.8 33.0 29.9
  fp32 B1 T257 H2 D16 scale1 p0.2        0.12 0.07 0.07 0.12 0.14 0.05 | 28.5 38.7 30.4 27.0
  fp32 B1 T1 H2 D64 scale1 p0.0          0.00 0.08 0.15 0.15 0.00 0.02 | 0.0 16.8 16.8 0.0
  fp32 B1 T1 H2 D64 scale1 p0.2          0.05 0.08 0.00 0.00 0.05 0.11 | 0.9 7.4 7.4 0.9
  fp32 B1 T2 H2 D64 scale1 p0.0          0.36 0.06 0.13 0.14 0.17 0.05 | 3.7 10.3 10.5 4.7
  fp32 B1 T2 H2 D64 scale1 p0.2          0.40 0.06 0.15 0.16 0.17 0.04 | 2.9 10.5 9.8 5.3
  fp32 B1 T31 H2 D64 scale1 p0.0         0.14 0.07 0.05 0.08 0.11 0.06 | 16.9 21.3 16.1 15.3
  fp32 B1 T31 H2 D64 scale1 p0.2         0.14 0.07 0.05 0.08 0.12 0.07 | 19.3 25.1 17.9 14.9
  fp32 B1 T32 H2 D64 scale1 p0.0         0.14 0.08 0.06 0.09 0.12 0.05 | 20.9 20.5 18.0 17.0
  fp32 B1 T32 H2 D64 scale1 p0.2         0.13 0.08 0.06 0.08 0.11 0.03 | 20.7 23.9 19.9 16.6
  fp32 B1 T33 H2 D64 scale1 p0.0         0.13 0.07 0.05 0.06 0.09 0.06 | 20.0 24.9 17.6 19.9
  fp32 B1 T33 H2 D64 scale1 p0.2         0.11 0.07 0.06 0.07 0.09 0.07 | 20.3 22.8 19.1 19.6
  fp32 B1 T63 H2 D64 scale1 p0.0         0.13 0.08 0.06 0.08 0.09 0.09 | 27.1 34.8 23.3 22.2
  fp32 B1 T63 H2 D64 scale1 p0.2         0.13 0.08 0.06 0.10 0.09 0.07 | 23.0 32.1 23.0 24.7
  fp32 B1 T64 H2 D64 scale1 p0.0         0.16 0.09 0.06 0.08 0.10 0.04 | 27.4 27.3 23.0 21.0
  fp32 B1 T64 H2 D64 scale1 p0.2         0.15 0.09 0.05 0.07 0.09 0.08 | 28.2 51.4 21.2 22.1
  fp32 B1 T65 H2 D64 scale1 p0.0         0.13 0.07 0.09 0.08 0.11 0.03 | 25.8 33.0 20.6 21.1
  fp32 B1 T65 H2 D64 scale1 p0.2         0.11 0.07 0.10 0.08 0.11 0.05 | 30.5 29.1 21.3 19.6
  fp32 B1 T127 H2 D64 scale1 p0.0        0.15 0.09 0.05 0.08 0.11 0.05 | 31.3 40.5 26.1 38.5
  fp32 B1 T127 H2 D64 scale1 p0.2        0.15 0.09 0.04 0.07 0.10 0.12 | 29.9 33.5 27.7 25.6
  fp32 B1 T128 H2 D64 scale1 p0.0        0.18 0.07 0.06 0.07 0.12 0.10 | 29.3 38.6 29.1 37.4
  fp32 B1 T128 H2 D64 scale1 p0.2        0.20 0.07 0.06 0.10 0.11 0.06 | 26.3 31.8 28.0 28.5
  fp32 B1 T129 H2 D64 scale1 p0.0        0.18 0.07 0.06 0.08 0.09 0.09 | 38.2 33.4 30.8 31.2
  fp32 B1 T129 H2 D64 scale1 p0.2        0.18 0.07 0.07 0.08 0.10 0.13 | 33.9 34.3 30.6 30.4
  fp32 B1 T255 H2 D64 scale1 p0.0        0.10 0.09 0.06 0.10 0.11 0.05 | 45.1 48.9 39.6 44.2
  fp32 B1 T255 H2 D64 scale1 p0.2        0.10 0.09 0.06 0.08 0.11 0.06 | 48.5 45.7 38.6 37.9
  fp32 B1 T256 H2 D64 scale1 p0.0        0.16 0.11 0.05 0.10 0.13 0.05 | 32.0 55.0 40.0 42.2
  fp32 B1 T256 H2 D64 scale1 p0.2        0.17 0.11 0.05 0.10 0.12 0.08 | 42.1 51.7 36.2 32.5
  fp32 B1 T257 H2 D64 scale1 p0.0        0.16 0.10 0.05 0.12 0.15 0.05 | 37.6 152.5 37.2 47.3
  fp32 B1 T257 H2 D64 scale1 p0.2        0.15 0.10 0.06 0.08 0.17 0.06 | 40.8 48.7 35.1 42.4
  bf16 B1 T1 H2 D16 scale1 p0.0          0.00 0.02 0.00 0.00 0.00 0.00 | 0.0 0.0 0.0 0.0
  bf16 B1 T1 H2 D16 scale1 p0.2          0.37 0.02 0.00 0.00 0.48 0.00 | 0.0 0.0 0.0 0.0
  bf16 B1 T2 H2 D16 scale1 p0.0          0.48 0.01 0.49 0.56 0.65 0.00 | 1.3 1.4 1.3 1.6
  bf16 B1 T2 H2 D16 scale1 p0.2          0.38 0.01 0.54 0.68 0.47 0.00 | 1.3 1.2 1.1 1.6
  bf16 B1 T31 H2 D16 scale1 p0.0         0.49 0.04 0.49 0.55 0.49 0.03 | 2.3 2.6 2.3 2.4
  bf16 B1 T31 H2 D16 scale1 p0.2         0.49 0.04 0.52 0.49 0.52 0.02 | 2.6 2.5 2.3 3.0
  bf16 B1 T32 H2 D16 scale1 p0.0         0.60 0.08 0.64 0.54 0.55 0.03 | 1.9 2.4 2.1 2.4
  bf16 B1 T32 H2 D16 scale1 p0.2         0.58 0.08 0.60 0.50 0.51 0.04 | 1.8 2.0 2.1 2.2
  bf16 B1 T33 H2 D16 scale1 p0.0         0.55 0.05 0.58 0.55 0.60 0.01 | 2.0 2.5 2.0 2.1
  bf16 B1 T33 H2 D16 scale1 p0.2         0.52 0.05 0.55 0.48 0.50 0.04 | 2.2 2.5 2.1 2.1
  bf16 B1 T63 H2 D16 scale1 p0.0         0.58 0.08 0.54 0.50 0.58 0.03 | 2.2 2.3 2.3 2.3
  bf16 B1 T63 H2 D16 scale1 p0.2         0.49 0.08 0.61 0.53 0.58 0.03 | 2.2 2.1 2.3 2.2
  bf16 B1 T64 H2 D16 scale1 p0.0         0.56 0.07 0.58 0.54 0.50 0.08 | 1.9 2.0 2.1 2.6
  bf16 B1 T64 H2 D16 scale1 p0.2         0.58 0.07 0.49 0.56 0.47 0.04 | 1.9 2.2 2.3 2.9
  bf16 B1 T65 H2 D16 scale1 p0.0         0.56 0.07 0.51 0.49 0.53 0.03 | 2.0 2.4 2.4 2.5
  bf16 B1 T65 H2 D16 scale1 p0.2         0.53 0.07 0.52 0.50 0.52 0.02 | 2.7 2.1 2.4 2.3
  bf16 B1 T127 H2 D16 scale1 p0.0        0.60 0.10 0.59 0.52 0.51 0.03 | 2.3 2.7 2.4 2.4
  bf16 B1 T127 H2 D16 scale1 p0.2        0.56 0.10 0.60 0.51 0.54 0.03 | 2.3 2.5 2.2 2.6
  bf16 B1 T128 H2 D16 scale1 p0.0        0.57 0.07 0.50 0.51 0.54 0.03 | 2.2 2.5 2.2 2.8
  bf16 B1 T128 H2 D16 scale1 p0.2        0.51 0.07 0.61 0.57 0.50 0.02 | 2.5 2.3 2.2 3.0
  bf16 B1 T129 H2 D16 scale1 p0.0        0.49 0.08 0.51 0.51 0.52 0.04 | 2.5 2.7 2.3 2.4
  bf16 B1 T129 H2 D16 scale1 p0.2        0.48 0.08 0.53 0.55 0.50 0.02 | 2.5 2.5 2.4 2.6
  bf16 B1 T255 H2 D16 scale1 p0.0        0.52 0.06 0.57 0.47 0.55 0.03 | 2.4 2.4 3.0 2.5
  bf16 B1 T255 H2 D16 scale1 p0.2        0.55 0.06 0.52 0.45 0.57 0.02 | 2.6 2.4 3.0 2.7
  bf16 B1 T256 H2 D16 scale1 p0.0        0.52 0.06 0.49 0.49 0.53 0.04 | 2.3 2.6 2.6 2.6
  bf16 B1 T256 H2 D16 scale1 p0.2        0.41 0.06 0.53 0.51 0.48 0.04 | 3.0 2.5 2.7 2.7
  bf16 B1 T257 H2 D16 scale1 p0.0        0.53 0.06 0.54 0.53 0.51 0.03 | 2.3 2.6 2.2 2.6
  bf16 B1 T257 H2 D16 scale1 p0.2        0.48 0.06 0.52 0.59 0.52 0.02 | 2.8 2.6 2.3 2.6
  bf16 B1 T1 H2 D64 scale1 p0.0          0.00 0.02 0.00 0.00 0.00 0.06 | 0.0 0.0 0.0 0.0
  bf16 B1 T1 H2 D64 scale1 p0.2          0.48 0.02 0.00 0.00 0.48 0.05 | 0.0 0.0 0.0 0.0
  bf16 B1 T2 H2 D64 scale1 p0.0          0.46 0.03 0.72 0.64 0.68 0.05 | 1.4 0.8 0.8 1.5
  bf16 B1 T2 H2 D64 scale1 p0.2          0.66 0.03 0.54 0.67 0.63 0.05 | 1.4 1.3 1.0 1.5
  bf16 B1 T31 H2 D64 scale1 p0.0         0.51 0.05 0.57 0.57 0.55 0.09 | 2.5 2.4 2.0 2.5
  bf16 B1 T31 H2 D64 scale1 p0.2         0.59 0.05 0.58 0.56 0.56 0.02 | 2.8 2.2 2.1 2.3
  bf16 B1 T32 H2 D64 scale1 p0.0         0.61 0.05 0.54 0.54 0.56 0.05 | 2.2 2.3 2.4 2.3
  bf16 B1 T32 H2 D64 scale1 p0.2         0.57 0.05 0.54 0.52 0.52 0.02 | 2.2 2.2 2.1 2.3
  bf16 B1 T33 H2 D64 scale1 p0.0         0.52 0.07 0.55 0.52 0.56 0.03 | 2.3 2.3 2.4 2.3
  bf16 B1 T33 H2 D64 scale1 p0.2         0.55 0.07 0.64 0.60 0.57 0.05 | 2.3 2.4 2.0 2.4
  bf16 B1 T63 H2 D64 scale1 p0.0         0.52 0.07 0.63 0.55 0.52 0.02 | 2.7 2.6 2.3 2.6
  bf16 B1 T63 H2 D64 scale1 p0.2         0.54 0.07 0.58 0.54 0.44 0.05 | 2.9 2.5 2.6 3.0
  bf16 B1 T64 H2 D64 scale1 p0.0         0.48 0.07 0.45 0.57 0.61 0.04 | 2.8 2.8 2.5 2.4
  bf16 B1 T64 H2 D64 scale1 p0.2         0.56 0.07 0.56 0.49 0.55 0.06 | 2.4 2.5 2.4 2.6
  bf16 B1 T65 H2 D64 scale1 p0.0         0.58 0.07 0.57 0.50 0.55 0.02 | 2.1 2.5 2.7 3.1
  bf16 B1 T65 H2 D64 scale1 p0.2         0.56 0.07 0.59 0.53 0.52 0.11 | 2.7 2.6 2.4 2.6
  bf16 B1 T127 H2 D64 scale1 p0.0        0.60 0.09 0.55 0.51 0.57 0.04 | 2.6 2.6 2.4 2.8
  bf16 B1 T127 H2 D64 scale1 p0.2        0.54 0.09 0.54 0.56 0.54 0.02 | 2.8 2.8 2.7 3.0
  bf16 B1 T128 H2 D64 scale1 p0.0        0.48 0.10 0.55 0.51 0.58 0.02 | 3.0 2.4 2.6 2.5
  bf16 B1 T128 H2 D64 scale1 p0.2        0.54 0.10 0.53 0.51 0.52 0.03 | 2.8 2.8 2.6 2.8
  bf16 B1 T129 H2 D64 scale1 p0.0        0.51 0.09 0.56 0.49 0.62 0.05 | 2.8 2.7 2.8 2.3
  bf16 B1 T129 H2 D64 scale1 p0.2        0.63 0.09 0.55 0.55 0.53 0.05 | 2.9 2.7 2.4 2.8
  bf16 B1 T255 H2 D64 scale1 p0.0        0.53 0.08 0.56 0.55 0.49 0.04 | 3.1 2.7 2.6 2.9
  bf16 B1 T255 H2 D64 scale1 p0.2        0.53 0.08 0.59 0.52 0.50 0.02 | 3.0 2.8 2.6 3.3
  bf16 B1 T256 H2 D64 scale1 p0.0        0.50 0.08 0.56 0.55 0.55 0.04 | 3.1 2.7 2.5 2.8
  bf16 B1 T256 H2 D64 scale1 p0.2        0.51 0.08 0.57 0.48 0.48 0.09 | 3.1 2.7 3.0 3.4
  bf16 B1 T257 H2 D64 scale1 p0.0        0.59 0.10 0.62 0.53 0.50 0.03 | 2.9 2.6 2.6 2.9
  bf16 B1 T257 H2 D64 scale1 p0.2        0.61 0.10 0.50 0.54 0.50 0.06 | 2.9 2.8 3.2 2.8
  fp32 B2 T333 H4 D64 scale1 p0.0        0.13 0.10 0.06 0.10 0.14 0.07 | 56.9 54.8 46.3 56.1
  fp32 B2 T333 H4 D64 scale1 p0.2        0.14 0.10 0.06 0.15 0.13 0.04 | 49.4 61.0 61.7 48.8
  bf16 B2 T333 H4 D64 scale1 p0.0        0.57 0.09 0.54 0.50 0.53 0.05 | 3.0 3.5 3.4 3.2
  bf16 B2 T333 H4 D64 scale1 p0.2        0.59 0.09 0.52 0.61 0.58 0.02 | 3.4 3.4 2.8 3.1
  fp32 B2 T333 H4 D128 scale1 p0.0       0.13 0.11 0.07 0.09 0.15 0.13 | 66.1 75.6 55.2 72.6
  fp32 B2 T333 H4 D128 scale1 p0.2       0.12 0.11 0.06 0.08 0.13 0.05 | 83.6 90.7 57.4 58.0
  bf16 B2 T333 H4 D128 scale1 p0.0       0.46 0.10 0.53 0.50 0.58 0.03 | 4.0 3.7 3.3 3.1
  bf16 B2 T333 H4 D128 scale1 p0.2       0.52 0.10 0.54 0.59 0.54 0.02 | 3.6 3.3 2.9 3.6
  bf16 B6 T333 H8 D16 scale1 p0.0        0.54 0.08 0.53 0.53 0.55 0.05 | 2.8 2.9 3.1 3.2
  bf16 B6 T333 H8 D16 scale1 p0.2        0.57 0.08 0.62 0.49 0.57 0.04 | 3.0 3.0 2.9 3.2
  bf16 B6 T333 H8 D32 scale1 p0.0        0.55 0.08 0.55 0.54 0.51 0.07 | 2.8 3.1 2.9 3.5
  bf16 B6 T333 H8 D32 scale1 p0.2        0.55 0.08 0.54 0.53 0.55 0.04 | 3.4 3.3 3.3 3.3
  fp32 B2 T333 H4 D64 scale0 p0.0        0.14 0.10 0.07 0.12 0.13 0.08 | 48.3 48.5 52.6 54.4
  fp32 B2 T333 H4 D64 scale0 p0.2        0.13 0.10 0.06 0.10 0.14 0.05 | 57.7 58.9 52.5 49.9
  bf16 B2 T333 H4 D64 scale0 p0.0        0.56 0.10 0.59 0.60 0.53 0.05 | 2.8 3.2 3.0 3.4
  bf16 B2 T333 H4 D64 scale0 p0.2        0.54 0.10 0.50 0.52 0.57 0.02 | 3.3 3.6 3.0 3.2
  bf16 B2 T333 H4 D16 scale1 p0.0        0.47 0.07 0.50 0.48 0.54 0.03 | 3.2 2.9 2.8 2.9
  bf16 B2 T333 H4 D16 scale1 p0.2        0.50 0.07 0.63 0.51 0.56 0.03 | 3.0 2.8 2.7 3.1
  bf16 B2 T333 H4 D32 scale1 p0.0        0.49 0.07 0.60 0.50 0.55 0.03 | 3.5 2.9 3.2 3.0
  bf16 B2 T333 H4 D32 scale1 p0.2        0.50 0.07 0.59 0.52 0.58 0.04 | 3.7 2.9 3.1 3.2
  bf16 B4 T333 H8 D16 scale1 p0.0        0.45 0.07 0.52 0.55 0.52 0.03 | 3.4 3.2 2.8 3.4
  bf16 B4 T333 H8 D16 scale1 p0.2        0.49 0.07 0.53 0.59 0.52 0.04 | 3.1 2.8 2.8 3.4
  bf16 B4 T333 H8 D32 scale1 p0.0        0.57 0.06 0.54 0.54 0.54 0.03 | 2.9 3.0 2.9 3.3
  bf16 B4 T333 H8 D32 scale1 p0.2        0.55 0.06 0.46 0.52 0.48 0.05 | 3.1 3.7 3.2 3.6
  bf16 B3 T384 H8 D64 scale1 p0.0 rstd   0.53 0.10 0.56 0.56 0.58 0.06 | 3.1 3.2 3.0 3.5
  bf16 B3 T384 H8 D64 scale1 p0.2 rstd   0.49 0.10 0.54 0.58 0.57 0.04 | 3.7 3.2 3.1 3.4
  bf16 B8 T1024 H8 D64 p0.0 randn        0.52 0.11 0.50 0.54 0.52 0.07 | 3.7 4.0 3.8 4.3
  bf16 B8 T1024 H8 D64 p0.0 planted      0.54 0.12 0.53 0.58 0.56 0.05 | 3.3 3.5 3.0 3.3
  bf16 B8 T1024 H8 D64 p0.1 randn        0.55 0.12 0.52 0.62 0.55 0.03 | 3.9 3.9 3.5 3.9
  bf16 B8 T1024 H8 D64 p0.1 planted      0.55 0.12 0.55 0.59 0.51 0.05 | 3.5 3.6 3.4 3.9
  bf16 B8 T2048 H8 D64 p0.0 randn        0.58 0.13 0.53 0.52 0.54 0.04 | 4.1 3.9 4.1 4.1
  bf16 B8 T2048 H8 D64 p0.0 planted      0.60 0.12 0.56 0.52 0.61 0.06 | 3.2 3.3 3.3 3.4
  bf16 B8 T2048 H8 D64 p0.1 randn        0.56 0.12 0.52 0.55 0.54 0.12 | 4.0 4.1 4.0 4.3
  bf16 B8 T2048 H8 D64 p0.1 planted      0.53 0.11 0.50 0.56 0.55 0.07 | 3.7 3.9 3.4 3.7
  fp32 B8 T1024 H8 D64 p0.1 randn        0.15 0.09 0.05 0.19 0.27 0.08 | 99.1 102.5 116.6 122.5
  fp32 B8 T1024 H8 D64 p0.1 planted      0.13 0.11 0.06 0.13 0.20 0.06 | 87.6 100.9 103.5 121.8
  bf16 B32 T1024 H8 D64 p0.1 randn       0.56 0.10 0.53 0.56 0.59 0.04 | 3.9 4.0 3.9 3.7
  bf16 B32 T1024 H8 D64 p0.1 planted     0.56 0.12 0.50 0.49 0.53 0.03 | 3.7 3.5 3.5 3.8
  bf16 B16 T1000 H8 D64 p0.1 randn       0.59 0.12 0.56 0.58 0.53 0.04 | 3.9 4.1 3.6 4.2
  bf16 B16 T1000 H8 D64 p0.1 planted     0.54 0.12 0.58 0.52 0.54 0.03 | 3.7 3.3 3.3 3.9
  bf16 B40 T640 H8 D64 p0.0 randn        0.57 0.09 0.55 0.52 0.55 0.03 | 3.8 3.8 3.7 3.9
  bf16 B40 T640 H8 D64 p0.0 planted      0.60 0.10 0.59 0.58 0.52 0.06 | 3.0 3.2 3.0 3.8
  bf16 B8 T2048 H16 D32 p0.1 randn       0.53 0.11 0.53 0.53 0.54 0.03 | 4.2 3.8 3.9 3.9
  bf16 B8 T2048 H16 D32 p0.1 planted     0.49 0.09 0.54 0.49 0.51 0.04 | 3.9 3.6 3.7 4.0
  fp32 B40 T512 H8 D64 p0.1 randn        0.13 0.09 0.05 0.16 0.19 0.12 | 55.4 56.5 71.1 87.1
  fp32 B40 T512 H8 D64 p0.1 planted      0.12 0.11 0.06 0.12 0.16 0.12 | 67.0 72.7 65.7 73.0
  bf16 B1 T1024 H16 D16 p0.1 randn       0.56 0.09 0.51 0.55 0.56 0.03 | 3.4 3.5 3.4 3.4
  bf16 B1 T1024 H16 D16 p0.1 planted     0.58 0.06 0.58 0.52 0.60 0.04 | 3.2 3.0 3.4 3.4
  bf16 B1 T1000 H16 D16 p0.0 randn       0.54 0.08 0.55 0.55 0.52 0.04 | 3.5 3.9 3.6 3.7
  bf16 B1 T1000 H16 D16 p0.0 planted     0.63 0.08 0.53 0.53 0.55 0.04 | 2.9 3.0 2.9 3.1
  bf16 B2 T600 H4 D32 p0.1 randn         0.54 0.09 0.58 0.55 0.56 0.06 | 3.8 3.7 3.7 3.6
  bf16 B2 T600 H4 D32 p0.1 planted       0.56 0.08 0.56 0.54 0.54 0.05 | 3.1 3.0 3.2 3.3
  bf16 B1 T96 H2 D16 p0.1 randn          0.47 0.08 0.46 0.58 0.55 0.03 | 2.9 3.3 2.6 2.6
  bf16 B1 T96 H2 D16 p0.1 planted        0.51 0.08 0.63 0.43 0.59 0.04 | 2.6 2.8 2.8 2.3
Mutation check (scratch builds, not kept; loops shortened only).  (1) The 128-row forward ends its key loop one 32-key sub-tile early for
the last query block: the 114 cases here that run a 128-row forward fail (the 24 key-split cases do not run it); 37 of the 68 older
attention tests fail as well, all short shapes, while three rows each of test_attention_full_length_many_groups (bf16 1024 with dropout,
both 2048) and test_attention_block_plans (1024, 1000, 2048) still passed their older assertions -- and now fail on o at 10 .. 38 limits.
(2) The dK/dV kernel skips its last query block: the same 114 cases fail, and 46 of the 68 older tests, every long row among them.
"""
import ctypes as C
import math

import pytest
import torch

import attention_bounds as AB
import test_gpu_ln_fused as L
from kernel_arena import Arena

pytestmark = pytest.mark.gpu

FP32, BF16 = AB.FP32, AB.BF16
F32 = torch.float32
P_DROP = [0.0, 0.2]
SEED, STREAM = 1234, 21

# (dtype, B, T, H, D, scale flag)
TILE_EDGE_T = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
TILE_EDGE_CASES = [(dt, 1, T, 2, D, 1) for dt in (FP32, BF16) for D in (16, 64) for T in TILE_EDGE_T]
ROWS_333_CASES = [(FP32, 2, 333, 4, 64, 1), (BF16, 2, 333, 4, 64, 1), (FP32, 2, 333, 4, 128, 1), (BF16, 2, 333, 4, 128, 1),
                  (BF16, 6, 333, 8, 16, 1), (BF16, 6, 333, 8, 32, 1),      # 144 blocks of the 128-row kind: not the key split
                  (FP32, 2, 333, 4, 64, 0), (BF16, 2, 333, 4, 64, 0)]      # scale = 0: raw scores
KEY_SPLIT_ONE_CASES = [(BF16, 2, 333, 4, 16, 1), (BF16, 2, 333, 4, 32, 1)]
KEY_SPLIT_TWO_CASES = [(BF16, 4, 333, 8, 16, 1), (BF16, 4, 333, 8, 32, 1)]
LN_ROWS_CASES = [(BF16, *L.ATTN_LN_ROWS_BT, L.ATTN_LN_ROWS_HEADS[0][1], L.ATTN_LN_ROWS_HEADS[0][0], 1)]


@pytest.fixture(scope="module")
def lib():
    from composer_amd import _lib
    l = _lib.load()
    _lib.require_gpu()
    return l


def ck(lib, rc):
    assert rc == 0, lib.cmp_last_error().decode()


def P(s):
    return C.c_void_p(s.ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_case(lib, dtype, B, T, H, D, sflag, p, ln=False):
    E = H * D
    dt = torch.bfloat16 if dtype == BF16 else F32
    scale = 1.0 / math.sqrt(D) if sflag else 1.0
    qkv_h, do_h = AB.attn_inputs(B, T, H, D, scale, seed=B * 1000 + T + D)
    esz = 2 if dtype == BF16 else 4
    ar = Arena("cuda", 8 * B * T * E * esz + 3 * 4 * B * H * T + (1 << 20))
    qkv = ar.operand(qkv_h, dt, B * T, 3 * E, 3 * E, name="qkv")
    do = ar.operand(do_h, dt, B * T, E, E, name="dO")
    rstd = None
    if ln:
        rstd = ar.vector(0.3 + 2.7 * torch.rand(B * T, generator=torch.Generator().manual_seed(T)), F32, name="rstd")
    o = ar.output(dt, B * T, E, E, name="o")
    lse = ar.output(F32, 1, B * H * T, B * H * T, name="lse")
    ar.arm()
    ck(lib, lib.cmp_k_attn_fwd(stream(), P(qkv), P(o), P(lse), B, T, H, D, sflag, dtype, p, SEED, STREAM))
    ar.check()
    ar.freeze(o, lse)
    dqkv = ar.output(dt, B * T, 3 * E, 3 * E, name="dqkv")
    delta = ar.output(F32, 1, B * H * T, B * H * T, name="delta")
    bias = ar.vector(torch.full((3 * E,), 2.0), F32, name="bias_grad", kind="acc")
    ar.arm()
    ck(lib, lib.cmp_attn_bwd_bias_next(P(bias)))
    if ln:
        ck(lib, lib.cmp_attn_bwd_ln_next(P(rstd)))
    ck(lib, lib.cmp_k_attn_bwd(stream(), P(qkv), P(o), P(do), P(lse), P(delta), P(dqkv), B, T, H, D, sflag, dtype, p, SEED, STREAM))
    ar.check()
    what = "attention %s B%d T%d H%d D%d scale%d p%.1f%s" % ("bf16" if dtype == BF16 else "fp32", B, T, H, D, sflag, p, " rstd" if ln else "")
    worst = AB.attn_check(qkv.host(), do.host(), o.host(), lse.host().reshape(-1), delta.host().reshape(-1), dqkv.host(), B, T, H, D,
                          dtype, p, scale, SEED, STREAM, AB.covering_groups(B, H), rstd=None if rstd is None else rstd.host().reshape(-1),
                          what=what, raise_on_fail=False)
    print(AB.figures(what, worst, dtype))                   # every figure of the case first, then the assertions
    AB.raise_first(worst)
    # the armed bias gradient: the column sums of the gradient this call computed, on top of the vector's contents (the tolerances of
    # test_gpu_kernels.test_attention_bias_gradient_paths, relative to the columns' absolute sums, plus one fp32 rounding of the
    # vector's own value, 2 + the sum: half a spacing of 2^-22 per [2, 4) it spans).  The rstd-scaled backward sums the UNSCALED
    # gradient (the column sums are taken in front of the rstd factor: test_gpu_ln_fused), so there the stored rows are divided by
    # their rstd again -- exact in float64, the store's bf16 rounding stays inside the 3e-3.
    got, have = dqkv.host().double(), bias.host().double().reshape(-1)
    if ln:
        got = got / rstd.host().double().reshape(-1, 1)
    err = (have - (got.sum(0) + 2.0)).abs()
    assert bool((err <= 3e-3 * got.abs().sum(0) + 2.0 ** -23 * have.abs().clamp_min(2.0)).all()), err.max().item()
    return worst


@pytest.mark.parametrize("p", P_DROP)
@pytest.mark.parametrize("dtype,B,T,H,D,sflag", TILE_EDGE_CASES)
def test_tile_edge_lengths(lib, dtype, B, T, H, D, sflag, p):
    run_case(lib, dtype, B, T, H, D, sflag, p)


@pytest.mark.parametrize("p", P_DROP)
@pytest.mark.parametrize("dtype,B,T,H,D,sflag", ROWS_333_CASES)
def test_128_row_kernels_at_333(lib, dtype, B, T, H, D, sflag, p):
    run_case(lib, dtype, B, T, H, D, sflag, p)


@pytest.mark.parametrize("p", P_DROP)
@pytest.mark.parametrize("dtype,B,T,H,D,sflag", KEY_SPLIT_ONE_CASES)
def test_key_split_one_launch(lib, dtype, B, T, H, D, sflag, p):
    run_case(lib, dtype, B, T, H, D, sflag, p)


@pytest.mark.parametrize("p", P_DROP)
@pytest.mark.parametrize("dtype,B,T,H,D,sflag", KEY_SPLIT_TWO_CASES)
def test_key_split_two_launches(lib, dtype, B, T, H, D, sflag, p):
    run_case(lib, dtype, B, T, H, D, sflag, p)


@pytest.mark.parametrize("p", P_DROP)
@pytest.mark.parametrize("dtype,B,T,H,D,sflag", LN_ROWS_CASES)
def test_rstd_scaled_backward(lib, dtype, B, T, H, D, sflag, p):
    run_case(lib, dtype, B, T, H, D, sflag, p, ln=True)
