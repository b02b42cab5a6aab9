"""The GEMM case table and its host-side checks (no GPU): which launch plan every case lands on, and that the table
reaches every plan `make_plan` / `plan_order` (csrc/gemm.hip) can produce.

`GEMM_CASES` is THE list of plain-GEMM launches the suite pins: tests/test_gpu_gemm.py runs every row exactly on the GPU,
this file asserts, through the host-side query `nsgp_gemm_plan`, the plan each row is expected to run.  A heuristic change
that moves a row fails `test_every_case_lands_on_its_expected_plan`; it is answered by correcting that row's plan AND
adding a row for the plan it left (which `test_the_table_reaches_every_reachable_plan` then demands), never by dropping one.

Exactness bound of the table (asserted per row in `test_every_case_keeps_integer_arithmetic_exact`): operands hold
integers in -3..4, C0 integers in -8..8, alpha in {1, -1, 0.5, -2}, beta in {0, 1, -2}, the diagonal may be halved.  Every
partial sum of the products is an integer of magnitude <= 16 K; alpha and the halving scale it by a power of two, down to a
multiple of 1/4; beta C0 adds an integer of magnitude <= 16.  So every intermediate, in any summation order, split or tile,
is a multiple of 1/4 of magnitude <= 2 * 16 K + 16: exact in float32 as long as 4 (32 K + 16) < 2^24 (K <= 131000), and the
float64 product of the same operands is the exact answer for both dtypes.
"""
import collections
import ctypes
import itertools

import pytest
import torch

AL, AU, BL, BU, CL, NS, NF, HD = 1, 2, 4, 8, 16, 32, 64, 128     # NSGP_GEMM_* of include/nsgp.h
TRI = AL | AU | BL | BU | CL
ALPHAS, BETAS = (1.0, -1.0, 0.5, -2.0), (0.0, 1.0, -2.0)
DTYPES = {'f32': torch.float32, 'f64': torch.float64}

# plan = (tile_m, tile_n, ksplit, kper, whole, xcd_chunk, batch_perm, grid_x, grid_y): fields 0..8 of nsgp_gemm_plan.
# The flags describe op(A) / op(B) (include/nsgp.h), whatever ta / tb say about how they are stored.
# nb: 0 = 2-D operands, n >= 1 = a batch of n (3-D operands).
# nb2 > 1: the two-level batch nsgp_trtri passes (nb x nb2 diagonal blocks of nb square matrices; through the C ABI only).
# va / vb: how the operand is stored, see `operand_view`.
Case = collections.namedtuple('Case', 'name dt M N K nb ta tb flags alpha beta va vb plan nb2')


def C(name, dt, M, N, K, nb, ta, tb, flags, alpha, beta, va, vb, plan, nb2=1):
    return Case(name, dt, M, N, K, nb, bool(ta), bool(tb), flags, alpha, beta, va, vb, tuple(plan), nb2)


# GEMM_CASES_BEGIN
GEMM_CASES = [
    # ---- all four operand layouts, with vector loads (c) and without (ptr1), per tile shape and dtype
    C('f32-64-nn-c', 'f32', 128, 192, 64, 0, 0, 0, 0, 1.0, 0.0, 'c', 'c', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f32-64-nn-ptr1', 'f32', 128, 192, 64, 0, 0, 0, 0, 1.0, 1.0, 'ptr1', 'ptr1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f32-64-nt-c', 'f32', 128, 192, 64, 0, 0, 1, 0, 1.0, -2.0, 'c', 'c', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f32-64-nt-ptr1', 'f32', 128, 192, 64, 0, 0, 1, 0, -1.0, 0.0, 'ptr1', 'ptr1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f32-64-tn-c', 'f32', 128, 192, 64, 0, 1, 0, 0, -1.0, 1.0, 'c', 'c', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f32-64-tn-ptr1', 'f32', 128, 192, 64, 0, 1, 0, 0, -1.0, -2.0, 'ptr1', 'ptr1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f32-64-tt-c', 'f32', 128, 192, 64, 0, 1, 1, 0, 0.5, 0.0, 'c', 'c', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f32-64-tt-ptr1', 'f32', 128, 192, 64, 0, 1, 1, 0, 0.5, 1.0, 'ptr1', 'ptr1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f64-64-nn-c', 'f64', 128, 192, 64, 0, 0, 0, 0, 0.5, -2.0, 'c', 'c', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f64-64-nn-ptr1', 'f64', 128, 192, 64, 0, 0, 0, 0, -2.0, 0.0, 'ptr1', 'ptr1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f64-64-nt-c', 'f64', 128, 192, 64, 0, 0, 1, 0, -2.0, 1.0, 'c', 'c', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f64-64-nt-ptr1', 'f64', 128, 192, 64, 0, 0, 1, 0, -2.0, -2.0, 'ptr1', 'ptr1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f64-64-tn-c', 'f64', 128, 192, 64, 0, 1, 0, 0, 1.0, 0.0, 'c', 'c', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f64-64-tn-ptr1', 'f64', 128, 192, 64, 0, 1, 0, 0, 1.0, 1.0, 'ptr1', 'ptr1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f64-64-tt-c', 'f64', 128, 192, 64, 0, 1, 1, 0, 1.0, -2.0, 'c', 'c', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f64-64-tt-ptr1', 'f64', 128, 192, 64, 0, 1, 1, 0, -1.0, 0.0, 'ptr1', 'ptr1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f32-big-nn-c', 'f32', 2048, 2048, 64, 0, 0, 0, 0, -1.0, 1.0, 'c', 'c', (128, 128, 1, 64, 1, 0, 0, 256, 1)),
    C('f32-big-nn-ptr1', 'f32', 2048, 2048, 64, 0, 0, 0, 0, -1.0, -2.0, 'ptr1', 'ptr1', (128, 128, 1, 64, 0, 0, 0, 256, 1)),
    C('f32-big-nt-c', 'f32', 2048, 2048, 64, 0, 0, 1, 0, 0.5, 0.0, 'c', 'c', (128, 128, 1, 64, 1, 0, 0, 256, 1)),
    C('f32-big-nt-ptr1', 'f32', 2048, 2048, 64, 0, 0, 1, 0, 0.5, 1.0, 'ptr1', 'ptr1', (128, 128, 1, 64, 0, 0, 0, 256, 1)),
    C('f32-big-tn-c', 'f32', 2048, 2048, 64, 0, 1, 0, 0, 0.5, -2.0, 'c', 'c', (128, 128, 1, 64, 1, 0, 0, 256, 1)),
    C('f32-big-tn-ptr1', 'f32', 2048, 2048, 64, 0, 1, 0, 0, -2.0, 0.0, 'ptr1', 'ptr1', (128, 128, 1, 64, 0, 0, 0, 256, 1)),
    C('f32-big-tt-c', 'f32', 2048, 2048, 64, 0, 1, 1, 0, -2.0, 1.0, 'c', 'c', (128, 128, 1, 64, 1, 0, 0, 256, 1)),
    C('f32-big-tt-ptr1', 'f32', 2048, 2048, 64, 0, 1, 1, 0, -2.0, -2.0, 'ptr1', 'ptr1', (128, 128, 1, 64, 0, 0, 0, 256, 1)),
    C('f32-narrow-nn-c', 'f32', 256, 16384, 256, 0, 0, 0, AL, 1.0, 0.0, 'c', 'c', (128, 64, 1, 256, 1, 0, 3, 512, 1)),
    C('f32-narrow-nn-ptr1', 'f32', 256, 16384, 256, 0, 0, 0, AL, 1.0, 1.0, 'ptr1', 'ptr1', (128, 64, 1, 256, 0, 0, 3, 512, 1)),
    C('f32-narrow-nt-c', 'f32', 256, 16384, 256, 0, 0, 1, AL, 1.0, -2.0, 'c', 'c', (128, 64, 1, 256, 1, 0, 3, 512, 1)),
    C('f32-narrow-nt-ptr1', 'f32', 256, 16384, 256, 0, 0, 1, AL, -1.0, 0.0, 'ptr1', 'ptr1', (128, 64, 1, 256, 0, 0, 3, 512, 1)),
    C('f32-narrow-tn-c', 'f32', 256, 16384, 256, 0, 1, 0, AL, -1.0, 1.0, 'c', 'c', (128, 64, 1, 256, 1, 0, 3, 512, 1)),
    C('f32-narrow-tn-ptr1', 'f32', 256, 16384, 256, 0, 1, 0, AL, -1.0, -2.0, 'ptr1', 'ptr1', (128, 64, 1, 256, 0, 0, 3, 512, 1)),
    C('f32-narrow-tt-c', 'f32', 256, 16384, 256, 0, 1, 1, AL, 0.5, 0.0, 'c', 'c', (128, 64, 1, 256, 1, 0, 3, 512, 1)),
    C('f32-narrow-tt-ptr1', 'f32', 256, 16384, 256, 0, 1, 1, AL, 0.5, 1.0, 'ptr1', 'ptr1', (128, 64, 1, 256, 0, 0, 3, 512, 1)),
    # ---- ragged shapes (bounds code by shape, not by alignment)
    C('f32-ragged', 'f32', 250, 315, 130, 0, 0, 0, 0, 0.5, -2.0, 'c', 'c', (64, 64, 1, 160, 0, 0, 0, 20, 1)),
    C('f64-ragged', 'f64', 250, 315, 130, 0, 0, 0, 0, -2.0, 0.0, 'c', 'c', (64, 64, 1, 160, 0, 0, 0, 20, 1)),
    C('f32-ragged-tt', 'f32', 250, 315, 130, 0, 1, 1, 0, -2.0, 1.0, 'c', 'c', (64, 64, 1, 160, 0, 0, 0, 20, 1)),
    C('f64-ragged-tt', 'f64', 250, 315, 130, 0, 1, 1, 0, -2.0, -2.0, 'c', 'c', (64, 64, 1, 160, 0, 0, 0, 20, 1)),
    C('f32-tiny', 'f32', 1, 7, 3, 0, 0, 0, 0, 1.0, 0.0, 'c', 'c', (64, 64, 1, 32, 0, 0, 0, 1, 1)),
    C('f64-tiny', 'f64', 1, 7, 3, 0, 0, 0, 0, 1.0, 1.0, 'c', 'c', (64, 64, 1, 32, 0, 0, 0, 1, 1)),
    C('f32-big-ragged', 'f32', 2000, 2100, 70, 0, 0, 1, 0, 1.0, -2.0, 'c', 'c', (128, 128, 1, 96, 0, 0, 0, 272, 1)),
    C('f32-narrow-ragged', 'f32', 250, 16400, 250, 0, 0, 0, AL, -1.0, 0.0, 'c', 'c', (128, 64, 1, 256, 0, 0, 3, 514, 1)),
    # ---- one row per plan key the planner can produce (tile order remaps, split-K with and without the XCD chunks)
    C('f32-perm1-c', 'f32', 64, 64, 16, 2, 0, 0, AL, -1.0, 1.0, 'c', 'c', (64, 64, 1, 32, 1, 0, 1, 1, 2)),
    C('f32-perm3-c', 'f32', 1024, 2048, 16, 0, 0, 0, AL, -1.0, -2.0, 'c', 'c', (64, 64, 1, 32, 1, 0, 3, 512, 1)),
    C('f32-split-c', 'f32', 64, 64, 512, 0, 0, 1, 0, 0.5, 0.0, 'c', 'c', (64, 64, 2, 256, 1, 0, 0, 1, 2)),
    C('f32-split-xcd-c', 'f32', 64, 256, 4096, 0, 0, 1, 0, 0.5, 1.0, 'c', 'c', (64, 64, 16, 256, 1, 1, 0, 4, 16)),
    C('f64-perm1-c', 'f64', 64, 64, 16, 2, 0, 0, AL, 0.5, -2.0, 'c', 'c', (64, 64, 1, 32, 1, 0, 1, 1, 2)),
    C('f64-perm3-c', 'f64', 1024, 2048, 16, 0, 0, 0, AL, -2.0, 0.0, 'c', 'c', (64, 64, 1, 32, 1, 0, 3, 512, 1)),
    C('f64-split-c', 'f64', 64, 64, 512, 0, 0, 1, 0, -2.0, 1.0, 'c', 'c', (64, 64, 2, 256, 1, 0, 0, 1, 2)),
    C('f64-split-xcd-c', 'f64', 64, 256, 4096, 0, 0, 1, 0, -2.0, -2.0, 'c', 'c', (64, 64, 16, 256, 1, 1, 0, 4, 16)),
    C('f64-perm2-c', 'f64', 1024, 2048, 16, 2, 0, 0, AL, 1.0, 0.0, 'c', 'c', (64, 64, 1, 32, 1, 0, 2, 512, 2)),
    C('f32-narrow-perm0-c', 'f32', 2048, 4096, 32, 0, 0, 0, AL, 1.0, 1.0, 'c', 'c', (128, 64, 1, 32, 1, 0, 0, 1024, 1)),
    C('f32-narrow-perm1-c', 'f32', 1024, 2048, 32, 2, 0, 0, AL, 1.0, -2.0, 'c', 'c', (128, 64, 1, 32, 1, 0, 1, 256, 2)),
    C('f32-narrow-perm2-c', 'f32', 1024, 4096, 32, 2, 0, 0, AL, -1.0, 0.0, 'c', 'c', (128, 64, 1, 32, 1, 0, 2, 512, 2)),
    C('f32-narrow-perm3-c', 'f32', 1024, 4096, 32, 0, 0, 0, AL, -1.0, 1.0, 'c', 'c', (128, 64, 1, 32, 1, 0, 3, 512, 1)),
    C('f32-big-perm0-batched-c', 'f32', 1024, 2048, 32, 2, 0, 0, 0, -1.0, -2.0, 'c', 'c', (128, 128, 1, 32, 1, 0, 0, 128, 2)),
    C('f32-big-perm1-c', 'f32', 1024, 2048, 32, 2, 0, 0, BL, 0.5, 0.0, 'c', 'c', (128, 128, 1, 32, 1, 0, 1, 128, 2)),
    C('f32-big-perm2-c', 'f32', 1024, 4096, 32, 3, 0, 0, AL, 0.5, 1.0, 'c', 'c', (128, 128, 1, 32, 1, 0, 2, 256, 3)),
    C('f32-big-perm3-c', 'f32', 2048, 4096, 32, 0, 0, 0, BL, 0.5, -2.0, 'c', 'c', (128, 128, 1, 32, 1, 0, 3, 512, 1)),
    C('f32-big-split-xcd-c', 'f32', 256, 1024, 4096, 0, 0, 1, 0, -2.0, 0.0, 'c', 'c', (128, 128, 16, 256, 1, 1, 0, 16, 16)),
    C('f32-perm1-ptr1', 'f32', 64, 64, 16, 2, 0, 0, AL, -2.0, 1.0, 'ptr1', 'ptr1', (64, 64, 1, 32, 0, 0, 1, 1, 2)),
    C('f32-perm3-ptr1', 'f32', 1024, 2048, 16, 0, 0, 0, AL, -2.0, -2.0, 'ptr1', 'ptr1', (64, 64, 1, 32, 0, 0, 3, 512, 1)),
    C('f32-split-ptr1', 'f32', 64, 64, 512, 0, 0, 1, 0, 1.0, 0.0, 'ptr1', 'ptr1', (64, 64, 2, 256, 0, 0, 0, 1, 2)),
    C('f32-split-xcd-ptr1', 'f32', 64, 256, 4096, 0, 0, 1, 0, 1.0, 1.0, 'ptr1', 'ptr1', (64, 64, 16, 256, 0, 1, 0, 4, 16)),
    C('f64-perm1-ptr1', 'f64', 64, 64, 16, 2, 0, 0, AL, 1.0, -2.0, 'ptr1', 'ptr1', (64, 64, 1, 32, 0, 0, 1, 1, 2)),
    C('f64-perm3-ptr1', 'f64', 1024, 2048, 16, 0, 0, 0, AL, -1.0, 0.0, 'ptr1', 'ptr1', (64, 64, 1, 32, 0, 0, 3, 512, 1)),
    C('f64-split-ptr1', 'f64', 64, 64, 512, 0, 0, 1, 0, -1.0, 1.0, 'ptr1', 'ptr1', (64, 64, 2, 256, 0, 0, 0, 1, 2)),
    C('f64-split-xcd-ptr1', 'f64', 64, 256, 4096, 0, 0, 1, 0, -1.0, -2.0, 'ptr1', 'ptr1', (64, 64, 16, 256, 0, 1, 0, 4, 16)),
    C('f64-perm2-ptr1', 'f64', 1024, 2048, 16, 2, 0, 0, AL, 0.5, 0.0, 'ptr1', 'ptr1', (64, 64, 1, 32, 0, 0, 2, 512, 2)),
    C('f32-narrow-perm0-ptr1', 'f32', 2048, 4096, 32, 0, 0, 0, AL, 0.5, 1.0, 'ptr1', 'ptr1', (128, 64, 1, 32, 0, 0, 0, 1024, 1)),
    C('f32-narrow-perm1-ptr1', 'f32', 1024, 2048, 32, 2, 0, 0, AL, 0.5, -2.0, 'ptr1', 'ptr1', (128, 64, 1, 32, 0, 0, 1, 256, 2)),
    C('f32-narrow-perm2-ptr1', 'f32', 1024, 4096, 32, 2, 0, 0, AL, -2.0, 0.0, 'ptr1', 'ptr1', (128, 64, 1, 32, 0, 0, 2, 512, 2)),
    C('f32-narrow-perm3-ptr1', 'f32', 1024, 4096, 32, 0, 0, 0, AL, -2.0, 1.0, 'ptr1', 'ptr1', (128, 64, 1, 32, 0, 0, 3, 512, 1)),
    C('f32-big-perm0-batched-ptr1', 'f32', 1024, 2048, 32, 2, 0, 0, 0, -2.0, -2.0, 'ptr1', 'ptr1', (128, 128, 1, 32, 0, 0, 0, 128, 2)),
    C('f32-big-perm1-ptr1', 'f32', 1024, 2048, 32, 2, 0, 0, BL, 1.0, 0.0, 'ptr1', 'ptr1', (128, 128, 1, 32, 0, 0, 1, 128, 2)),
    C('f32-big-perm2-ptr1', 'f32', 1024, 4096, 32, 3, 0, 0, AL, 1.0, 1.0, 'ptr1', 'ptr1', (128, 128, 1, 32, 0, 0, 2, 256, 3)),
    C('f32-big-perm3-ptr1', 'f32', 2048, 4096, 32, 0, 0, 0, BL, 1.0, -2.0, 'ptr1', 'ptr1', (128, 128, 1, 32, 0, 0, 3, 512, 1)),
    C('f32-big-split-xcd-ptr1', 'f32', 256, 1024, 4096, 0, 0, 1, 0, -1.0, 0.0, 'ptr1', 'ptr1', (128, 128, 16, 256, 0, 1, 0, 16, 16)),
    # ---- every triangle flag alone: single pass (ragged), split-K, and the same shape with NO_SPLITK
    C('f32-AL-200', 'f32', 200, 200, 200, 0, 0, 0, AL, -1.0, 1.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 16, 1)),
    C('f64-AL-200', 'f64', 200, 200, 200, 0, 0, 0, AL, -1.0, -2.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 16, 1)),
    C('f32-AL-split', 'f32', 1024, 1024, 1024, 0, 0, 0, AL, 0.5, 0.0, 'c', 'c', (128, 128, 4, 256, 1, 1, 0, 64, 4)),
    C('f64-AL-split', 'f64', 1024, 1024, 1024, 0, 0, 0, AL, 0.5, 1.0, 'c', 'c', (64, 64, 3, 352, 1, 1, 0, 256, 3)),
    C('f32-AL-nosplit', 'f32', 1024, 1024, 1024, 0, 0, 0, AL | NS, 0.5, -2.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 0, 256, 1)),
    C('f64-AL-nosplit', 'f64', 1024, 1024, 1024, 0, 0, 0, AL | NS, -2.0, 0.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 0, 256, 1)),
    C('f32-AU-200', 'f32', 200, 200, 200, 0, 0, 0, AU, -2.0, 1.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 16, 1)),
    C('f64-AU-200', 'f64', 200, 200, 200, 0, 0, 0, AU, -2.0, -2.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 16, 1)),
    C('f32-AU-split', 'f32', 1024, 1024, 1024, 0, 0, 0, AU, 1.0, 0.0, 'c', 'c', (128, 128, 4, 256, 1, 1, 0, 64, 4)),
    C('f64-AU-split', 'f64', 1024, 1024, 1024, 0, 0, 0, AU, 1.0, 1.0, 'c', 'c', (64, 64, 3, 352, 1, 1, 0, 256, 3)),
    C('f32-AU-nosplit', 'f32', 1024, 1024, 1024, 0, 0, 0, AU | NS, 1.0, -2.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 0, 256, 1)),
    C('f64-AU-nosplit', 'f64', 1024, 1024, 1024, 0, 0, 0, AU | NS, -1.0, 0.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 0, 256, 1)),
    C('f32-BL-200', 'f32', 200, 200, 200, 0, 0, 0, BL, -1.0, 1.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 16, 1)),
    C('f64-BL-200', 'f64', 200, 200, 200, 0, 0, 0, BL, -1.0, -2.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 16, 1)),
    C('f32-BL-split', 'f32', 1024, 1024, 1024, 0, 0, 0, BL, 0.5, 0.0, 'c', 'c', (128, 128, 4, 256, 1, 1, 0, 64, 4)),
    C('f64-BL-split', 'f64', 1024, 1024, 1024, 0, 0, 0, BL, 0.5, 1.0, 'c', 'c', (64, 64, 3, 352, 1, 1, 0, 256, 3)),
    C('f32-BL-nosplit', 'f32', 1024, 1024, 1024, 0, 0, 0, BL | NS, 0.5, -2.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 0, 256, 1)),
    C('f64-BL-nosplit', 'f64', 1024, 1024, 1024, 0, 0, 0, BL | NS, -2.0, 0.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 0, 256, 1)),
    C('f32-BU-200', 'f32', 200, 200, 200, 0, 0, 0, BU, -2.0, 1.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 16, 1)),
    C('f64-BU-200', 'f64', 200, 200, 200, 0, 0, 0, BU, -2.0, -2.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 16, 1)),
    C('f32-BU-split', 'f32', 1024, 1024, 1024, 0, 0, 0, BU, 1.0, 0.0, 'c', 'c', (128, 128, 4, 256, 1, 1, 0, 64, 4)),
    C('f64-BU-split', 'f64', 1024, 1024, 1024, 0, 0, 0, BU, 1.0, 1.0, 'c', 'c', (64, 64, 3, 352, 1, 1, 0, 256, 3)),
    C('f32-BU-nosplit', 'f32', 1024, 1024, 1024, 0, 0, 0, BU | NS, 1.0, -2.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 0, 256, 1)),
    C('f64-BU-nosplit', 'f64', 1024, 1024, 1024, 0, 0, 0, BU | NS, -1.0, 0.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 0, 256, 1)),
    C('f32-CL-200', 'f32', 200, 200, 200, 0, 0, 0, CL, -1.0, 1.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 10, 1)),
    C('f64-CL-200', 'f64', 200, 200, 200, 0, 0, 0, CL, -1.0, -2.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 10, 1)),
    C('f32-CL-split', 'f32', 192, 192, 2048, 0, 0, 1, CL, 0.5, 0.0, 'c', 'c', (64, 64, 8, 256, 1, 0, 0, 6, 8)),
    C('f64-CL-split', 'f64', 192, 192, 2048, 0, 0, 1, CL, 0.5, 1.0, 'c', 'c', (64, 64, 8, 256, 1, 0, 0, 6, 8)),
    C('f32-CL-nosplit', 'f32', 1024, 1024, 1024, 0, 0, 0, CL | NS, 0.5, -2.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 0, 136, 1)),
    C('f64-CL-nosplit', 'f64', 1024, 1024, 1024, 0, 0, 0, CL | NS, -2.0, 0.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 0, 136, 1)),
    # ---- the Cholesky adjoint (svgp.py WhitenFn.backward, ops.py chol_inv backward): Phi, Phi W, W^T T
    C('f32-adj-phi-200', 'f32', 200, 200, 200, 0, 0, 1, AL | BU | CL | NF | HD, -2.0, 1.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 10, 1)),
    C('f64-adj-phi-200', 'f64', 200, 200, 200, 0, 0, 1, AL | BU | CL | NF | HD, -2.0, -2.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 10, 1)),
    C('f32-adj-phi-nohalf-200', 'f32', 200, 200, 200, 0, 0, 1, AL | BU | CL | NF, 1.0, 0.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 10, 1)),
    C('f64-adj-phi-nohalf-200', 'f64', 200, 200, 200, 0, 0, 1, AL | BU | CL | NF, 1.0, 1.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 10, 1)),
    C('f32-adj-t-200', 'f32', 200, 200, 200, 0, 0, 0, AL | BL | CL | NF, 1.0, -2.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 10, 1)),
    C('f64-adj-t-200', 'f64', 200, 200, 200, 0, 0, 0, AL | BL | CL | NF, -1.0, 0.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 10, 1)),
    C('f32-adj-g-200', 'f32', 200, 200, 200, 0, 1, 0, AU | BL, -1.0, 0.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 16, 1)),
    C('f64-adj-g-200', 'f64', 200, 200, 200, 0, 1, 0, AU | BL, -1.0, 0.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 16, 1)),
    C('f32-adj-b-200', 'f32', 200, 200, 200, 0, 0, 1, AL | BU, -1.0, 1.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 16, 1)),
    C('f64-adj-b-200', 'f64', 200, 200, 200, 0, 0, 1, AL | BU, -1.0, -2.0, 'c', 'c', (64, 64, 1, 224, 0, 0, 0, 16, 1)),
    C('f32-adj-phi-1024', 'f32', 1024, 1024, 1024, 3, 0, 1, AL | BU | CL | NF | HD, 0.5, 0.0, 'c', 'c', (128, 128, 4, 256, 1, 1, 0, 36, 12)),
    C('f64-adj-phi-1024', 'f64', 1024, 1024, 1024, 3, 0, 1, AL | BU | CL | NF | HD, 0.5, 1.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 1, 136, 3)),
    C('f32-adj-phi-nohalf-1024', 'f32', 1024, 1024, 1024, 3, 0, 1, AL | BU | CL | NF, 0.5, -2.0, 'c', 'c', (128, 128, 4, 256, 1, 1, 0, 36, 12)),
    C('f64-adj-phi-nohalf-1024', 'f64', 1024, 1024, 1024, 3, 0, 1, AL | BU | CL | NF, -2.0, 0.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 1, 136, 3)),
    C('f32-adj-t-1024', 'f32', 1024, 1024, 1024, 3, 0, 0, AL | BL | CL | NF, -2.0, 1.0, 'c', 'c', (128, 128, 4, 256, 1, 1, 0, 36, 12)),
    C('f64-adj-t-1024', 'f64', 1024, 1024, 1024, 3, 0, 0, AL | BL | CL | NF, -2.0, -2.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 1, 136, 3)),
    C('f32-adj-g-1024', 'f32', 1024, 1024, 1024, 3, 1, 0, AU | BL, -1.0, 0.0, 'c', 'c', (128, 128, 2, 512, 1, 1, 0, 64, 6)),
    C('f64-adj-g-1024', 'f64', 1024, 1024, 1024, 3, 1, 0, AU | BL, -1.0, 0.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 1, 256, 3)),
    C('f32-adj-b-1024', 'f32', 1024, 1024, 1024, 3, 0, 1, AL | BU, 1.0, 0.0, 'c', 'c', (128, 128, 2, 512, 1, 1, 0, 64, 6)),
    C('f64-adj-b-1024', 'f64', 1024, 1024, 1024, 3, 0, 1, AL | BU, 1.0, 1.0, 'c', 'c', (64, 64, 1, 1024, 1, 0, 1, 256, 3)),
    C('f32-adj-phi-split', 'f32', 1024, 1024, 1024, 0, 0, 1, AL | BU | CL | NF | HD, 1.0, -2.0, 'c', 'c', (64, 64, 4, 256, 1, 1, 0, 136, 4)),
    C('f64-adj-phi-split', 'f64', 1024, 1024, 1024, 0, 0, 1, AL | BU | CL | NF | HD, -1.0, 0.0, 'c', 'c', (64, 64, 4, 256, 1, 1, 0, 136, 4)),
    C('f32-halfdiag-split-beta', 'f32', 128, 128, 4096, 0, 0, 1, CL | HD, 0.5, -2.0, 'c', 'c', (64, 64, 16, 256, 1, 0, 0, 3, 16)),
    C('f64-halfdiag-split-beta', 'f64', 128, 128, 4096, 0, 0, 1, CL | HD, 0.5, -2.0, 'c', 'c', (64, 64, 16, 256, 1, 0, 0, 3, 16)),
    C('f32-halfdiag-fill', 'f32', 200, 200, 64, 0, 0, 1, CL | HD, 0.5, 0.0, 'c', 'c', (64, 64, 1, 64, 0, 0, 0, 10, 1)),
    C('f64-halfdiag-fill', 'f64', 200, 200, 64, 0, 0, 1, CL | HD, 0.5, 0.0, 'c', 'c', (64, 64, 1, 64, 0, 0, 0, 10, 1)),
    # ---- C_LOWER: M > N, M < N, beta != 0 (single pass and split), filled and NOFILL
    C('f32-CL-tall', 'f32', 300, 200, 64, 0, 0, 0, CL, 1.0, 0.0, 'c', 'c', (64, 64, 1, 64, 0, 0, 0, 14, 1)),
    C('f64-CL-tall', 'f64', 300, 200, 64, 0, 0, 0, CL, 1.0, 0.0, 'c', 'c', (64, 64, 1, 64, 0, 0, 0, 14, 1)),
    C('f32-CL-wide', 'f32', 200, 300, 64, 0, 0, 0, CL, -2.0, 0.0, 'c', 'c', (64, 64, 1, 64, 0, 0, 0, 10, 1)),
    C('f64-CL-wide', 'f64', 200, 300, 64, 0, 0, 0, CL, -2.0, 0.0, 'c', 'c', (64, 64, 1, 64, 0, 0, 0, 10, 1)),
    C('f32-CL-tall-beta', 'f32', 300, 200, 64, 0, 0, 0, CL, 1.0, 1.0, 'c', 'c', (64, 64, 1, 64, 0, 0, 0, 14, 1)),
    C('f64-CL-tall-beta', 'f64', 300, 200, 64, 0, 0, 0, CL, 1.0, 1.0, 'c', 'c', (64, 64, 1, 64, 0, 0, 0, 14, 1)),
    C('f32-CL-wide-beta-nofill', 'f32', 200, 300, 64, 0, 0, 0, CL | NF, -1.0, -2.0, 'c', 'c', (64, 64, 1, 64, 0, 0, 0, 10, 1)),
    C('f64-CL-wide-beta-nofill', 'f64', 200, 300, 64, 0, 0, 0, CL | NF, -1.0, -2.0, 'c', 'c', (64, 64, 1, 64, 0, 0, 0, 10, 1)),
    C('f32-CL-split-beta', 'f32', 192, 192, 4096, 0, 0, 1, CL, 1.0, 1.0, 'c', 'c', (64, 64, 16, 256, 1, 1, 0, 6, 16)),
    C('f64-CL-split-beta', 'f64', 192, 192, 4096, 0, 0, 1, CL, 1.0, 1.0, 'c', 'c', (64, 64, 16, 256, 1, 1, 0, 6, 16)),
    C('f32-CL-split-nofill', 'f32', 192, 192, 4096, 0, 0, 1, CL | NF, 1.0, 0.0, 'c', 'c', (64, 64, 16, 256, 1, 1, 0, 6, 16)),
    C('f64-CL-split-nofill', 'f64', 192, 192, 4096, 0, 0, 1, CL | NF, 1.0, 0.0, 'c', 'c', (64, 64, 16, 256, 1, 1, 0, 6, 16)),
    C('f32-CL-batched-tall', 'f32', 300, 200, 64, 3, 0, 1, CL, 1.0, 0.0, 'c', 'c', (64, 64, 1, 64, 0, 0, 1, 14, 3)),
    C('f64-CL-batched-tall', 'f64', 300, 200, 64, 3, 0, 1, CL, 1.0, 0.0, 'c', 'c', (64, 64, 1, 64, 0, 0, 1, 14, 3)),
    # ---- production shapes: the projections of the SVGP layer with and without NO_SPLITK, their adjoints, a column vector
    C('f32-proj-4096-AL', 'f32', 1024, 4096, 1024, 0, 0, 0, AL, 1.0, 0.0, 'c', 'c', (128, 128, 2, 512, 1, 1, 0, 256, 2)),
    C('f32-proj-4096-AL-nosplit', 'f32', 1024, 4096, 1024, 0, 0, 0, AL | NS, 1.0, 0.0, 'c', 'c', (128, 64, 1, 1024, 1, 0, 3, 512, 1)),
    C('f32-proj-4096-AU-nosplit', 'f32', 1024, 4096, 1024, 0, 1, 0, AU | NS, 1.0, 0.0, 'c', 'c', (128, 64, 1, 1024, 1, 0, 3, 512, 1)),
    C('f32-proj-5120-AL', 'f32', 1024, 5120, 1024, 0, 0, 0, AL, 1.0, 0.0, 'c', 'c', (128, 64, 1, 1024, 1, 0, 3, 640, 1)),
    C('f32-proj-5120-AL-nosplit', 'f32', 1024, 5120, 1024, 0, 0, 0, AL | NS, 1.0, 0.0, 'c', 'c', (128, 64, 1, 1024, 1, 0, 3, 640, 1)),
    C('f32-proj-5120-AU-nosplit', 'f32', 1024, 5120, 1024, 0, 1, 0, AU | NS, 1.0, 0.0, 'c', 'c', (128, 64, 1, 1024, 1, 0, 3, 640, 1)),
    C('f32-proj-4100-AL', 'f32', 1024, 4100, 1024, 0, 0, 0, AL, 1.0, 0.0, 'c', 'c', (128, 64, 1, 1024, 0, 0, 3, 520, 1)),
    C('f32-proj-4100-AL-nosplit', 'f32', 1024, 4100, 1024, 0, 0, 0, AL | NS, 1.0, 0.0, 'c', 'c', (128, 64, 1, 1024, 0, 0, 3, 520, 1)),
    C('f32-proj-4100-AU-nosplit', 'f32', 1024, 4100, 1024, 0, 1, 0, AU | NS, 1.0, 0.0, 'c', 'c', (128, 64, 1, 1024, 0, 0, 3, 520, 1)),
    C('f32-kzxbar', 'f32', 1024, 4096, 1024, 0, 1, 0, AU, 1.0, 0.0, 'c', 'c', (128, 128, 2, 512, 1, 1, 0, 256, 2)),
    C('f32-wbar', 'f32', 1024, 1024, 4096, 0, 0, 1, CL, 1.0, 0.0, 'c', 'c', (128, 128, 13, 320, 1, 1, 0, 36, 14)),
    C('f32-hidden-pair-nosplit', 'f32', 1024, 4096, 1024, 2, 0, 0, AL | NS, 1.0, 0.0, 'c', 'c', (128, 64, 1, 1024, 1, 0, 2, 512, 2)),
    C('f32-colvec', 'f32', 1024, 1, 1024, 0, 0, 0, AL, -1.0, 1.0, 'c', 'c', (64, 64, 4, 256, 0, 1, 0, 16, 4)),
    C('f64-colvec', 'f64', 1024, 1, 1024, 0, 0, 0, AL, -1.0, -2.0, 'c', 'c', (64, 64, 4, 256, 0, 1, 0, 16, 4)),
    C('f32-colvec-plain', 'f32', 300, 1, 700, 0, 0, 0, 0, 0.5, 0.0, 'c', 'c', (64, 64, 2, 352, 0, 0, 0, 5, 2)),
    C('f64-colvec-plain', 'f64', 300, 1, 700, 0, 0, 0, 0, 0.5, 1.0, 'c', 'c', (64, 64, 2, 352, 0, 0, 0, 5, 2)),
    # ---- the windows nsgp_potrf / nsgp_trtri pass (always NO_SPLITK, ldc > N).  potrf factors n <= 2048 in one level and calls
    # no GEMM; its first GEMM is the trailing update at n = 4096.  trtri at n = 1024: (s, s, s) blocks, s = 64 .. 512, as a two-level
    # batch; at n = 1100 also the ragged last pair (h = 12 at s = 64, h = 76 at s = 1024)
    C('f32-potrf-4096-trailing', 'f32', 2048, 2048, 2048, 0, 0, 1, CL | NS, -1.0, 1.0, 'win', 'win', (64, 64, 1, 2048, 1, 0, 3, 528, 1)),
    C('f64-potrf-4096-trailing', 'f64', 2048, 2048, 2048, 0, 0, 1, CL | NS, -1.0, 1.0, 'win', 'win', (64, 64, 1, 2048, 1, 0, 3, 528, 1)),
    C('f32-trtri-1024-s64-BL', 'f32', 64, 64, 64, 2, 0, 0, BL | NS, 1.0, 0.0, 'c', 'c', (64, 64, 1, 64, 1, 0, 1, 1, 16), nb2=8),
    C('f64-trtri-1024-s64-BL', 'f64', 64, 64, 64, 2, 0, 0, BL | NS, 1.0, 0.0, 'c', 'c', (64, 64, 1, 64, 1, 0, 1, 1, 16), nb2=8),
    C('f32-trtri-1024-s64-AL', 'f32', 64, 64, 64, 2, 0, 0, AL | NS, -1.0, 0.0, 'c', 'c', (64, 64, 1, 64, 1, 0, 1, 1, 16), nb2=8),
    C('f64-trtri-1024-s64-AL', 'f64', 64, 64, 64, 2, 0, 0, AL | NS, -1.0, 0.0, 'c', 'c', (64, 64, 1, 64, 1, 0, 1, 1, 16), nb2=8),
    C('f32-trtri-1024-s256-BL', 'f32', 256, 256, 256, 2, 0, 0, BL | NS, 1.0, 0.0, 'c', 'c', (64, 64, 1, 256, 1, 0, 1, 16, 4), nb2=2),
    C('f64-trtri-1024-s256-BL', 'f64', 256, 256, 256, 2, 0, 0, BL | NS, 1.0, 0.0, 'c', 'c', (64, 64, 1, 256, 1, 0, 1, 16, 4), nb2=2),
    C('f32-trtri-1024-s256-AL', 'f32', 256, 256, 256, 2, 0, 0, AL | NS, -1.0, 0.0, 'c', 'c', (64, 64, 1, 256, 1, 0, 1, 16, 4), nb2=2),
    C('f64-trtri-1024-s256-AL', 'f64', 256, 256, 256, 2, 0, 0, AL | NS, -1.0, 0.0, 'c', 'c', (64, 64, 1, 256, 1, 0, 1, 16, 4), nb2=2),
    C('f32-trtri-1024-s512-BL', 'f32', 512, 512, 512, 2, 0, 0, BL | NS, 1.0, 0.0, 'win', 'win', (64, 64, 1, 512, 1, 0, 1, 64, 2)),
    C('f64-trtri-1024-s512-BL', 'f64', 512, 512, 512, 2, 0, 0, BL | NS, 1.0, 0.0, 'win', 'win', (64, 64, 1, 512, 1, 0, 1, 64, 2)),
    C('f32-trtri-1024-s512-AL', 'f32', 512, 512, 512, 2, 0, 0, AL | NS, -1.0, 0.0, 'win', 'win', (64, 64, 1, 512, 1, 0, 1, 64, 2)),
    C('f64-trtri-1024-s512-AL', 'f64', 512, 512, 512, 2, 0, 0, AL | NS, -1.0, 0.0, 'win', 'win', (64, 64, 1, 512, 1, 0, 1, 64, 2)),
    C('f32-trtri-1100-s64-rem-BL', 'f32', 12, 64, 64, 2, 0, 0, BL | NS, 1.0, 0.0, 'win', 'win', (64, 64, 1, 64, 0, 0, 1, 1, 2)),
    C('f64-trtri-1100-s64-rem-BL', 'f64', 12, 64, 64, 2, 0, 0, BL | NS, 1.0, 0.0, 'win', 'win', (64, 64, 1, 64, 0, 0, 1, 1, 2)),
    C('f32-trtri-1100-s64-rem-AL', 'f32', 12, 64, 12, 2, 0, 0, AL | NS, -1.0, 0.0, 'win', 'win', (64, 64, 1, 32, 0, 0, 1, 1, 2)),
    C('f64-trtri-1100-s64-rem-AL', 'f64', 12, 64, 12, 2, 0, 0, AL | NS, -1.0, 0.0, 'win', 'win', (64, 64, 1, 32, 0, 0, 1, 1, 2)),
    C('f32-trtri-1100-s1024-rem-BL', 'f32', 76, 1024, 1024, 0, 0, 0, BL | NS, 1.0, 0.0, 'win', 'win', (64, 64, 1, 1024, 0, 0, 0, 32, 1)),
    C('f64-trtri-1100-s1024-rem-BL', 'f64', 76, 1024, 1024, 0, 0, 0, BL | NS, 1.0, 0.0, 'win', 'win', (64, 64, 1, 1024, 0, 0, 0, 32, 1)),
    C('f32-trtri-1100-s1024-rem-AL', 'f32', 76, 1024, 76, 0, 0, 0, AL | NS, -1.0, 0.0, 'win', 'win', (64, 64, 1, 96, 0, 0, 0, 32, 1)),
    C('f64-trtri-1100-s1024-rem-AL', 'f64', 76, 1024, 76, 0, 0, 0, AL | NS, -1.0, 0.0, 'win', 'win', (64, 64, 1, 96, 0, 0, 0, 32, 1)),
    # ---- operand views
    C('f32-win-nn', 'f32', 128, 192, 64, 0, 0, 0, 0, 0.5, -2.0, 'win', 'win', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f64-win-nn', 'f64', 128, 192, 64, 0, 0, 0, 0, -2.0, 0.0, 'win', 'win', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f32-win3d-nn', 'f32', 128, 192, 64, 2, 0, 0, 0, -2.0, 1.0, 'win', 'tcol', (64, 64, 1, 64, 0, 0, 0, 6, 2)),
    C('f64-win3d-nn', 'f64', 128, 192, 64, 2, 0, 0, 0, -2.0, -2.0, 'win', 'tcol', (64, 64, 1, 64, 0, 0, 0, 6, 2)),
    C('f32-win-nt', 'f32', 128, 192, 64, 0, 0, 1, 0, 1.0, 0.0, 'win', 'win', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f64-win-nt', 'f64', 128, 192, 64, 0, 0, 1, 0, 1.0, 1.0, 'win', 'win', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f32-win3d-nt', 'f32', 128, 192, 64, 2, 0, 1, 0, 1.0, -2.0, 'win', 'tcol', (64, 64, 1, 64, 0, 0, 0, 6, 2)),
    C('f64-win3d-nt', 'f64', 128, 192, 64, 2, 0, 1, 0, -1.0, 0.0, 'win', 'tcol', (64, 64, 1, 64, 0, 0, 0, 6, 2)),
    C('f32-win-tn', 'f32', 128, 192, 64, 0, 1, 0, 0, -1.0, 1.0, 'win', 'win', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f64-win-tn', 'f64', 128, 192, 64, 0, 1, 0, 0, -1.0, -2.0, 'win', 'win', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f32-win3d-tn', 'f32', 128, 192, 64, 2, 1, 0, 0, 0.5, 0.0, 'win', 'tcol', (64, 64, 1, 64, 0, 0, 0, 6, 2)),
    C('f64-win3d-tn', 'f64', 128, 192, 64, 2, 1, 0, 0, 0.5, 1.0, 'win', 'tcol', (64, 64, 1, 64, 0, 0, 0, 6, 2)),
    C('f32-win-tt', 'f32', 128, 192, 64, 0, 1, 1, 0, 0.5, -2.0, 'win', 'win', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f64-win-tt', 'f64', 128, 192, 64, 0, 1, 1, 0, -2.0, 0.0, 'win', 'win', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f32-win3d-tt', 'f32', 128, 192, 64, 2, 1, 1, 0, -2.0, 1.0, 'win', 'tcol', (64, 64, 1, 64, 0, 0, 0, 6, 2)),
    C('f64-win3d-tt', 'f64', 128, 192, 64, 2, 1, 1, 0, -2.0, -2.0, 'win', 'tcol', (64, 64, 1, 64, 0, 0, 0, 6, 2)),
    C('f32-ptr1-odd-row', 'f32', 126, 190, 62, 0, 0, 0, 0, 1.0, 0.0, 'ptr1', 'ptr1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f64-ptr1-odd-row', 'f64', 126, 190, 62, 0, 0, 0, 0, 1.0, 1.0, 'ptr1', 'ptr1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f32-row1-odd-row', 'f32', 126, 190, 62, 0, 0, 0, 0, 1.0, -2.0, 'row1', 'row1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f64-row1-odd-row', 'f64', 126, 190, 62, 0, 0, 0, 0, -1.0, 0.0, 'row1', 'row1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f32-row1-odd-row-tt', 'f32', 126, 190, 62, 0, 1, 1, 0, -1.0, 1.0, 'row1', 'row1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f64-row1-odd-row-tt', 'f64', 126, 190, 62, 0, 1, 1, 0, -1.0, -2.0, 'row1', 'row1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f32-ptr1-a-only', 'f32', 128, 192, 64, 0, 0, 0, 0, 0.5, 0.0, 'ptr1', 'c', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f64-ptr1-a-only', 'f64', 128, 192, 64, 0, 0, 0, 0, 0.5, 1.0, 'ptr1', 'c', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f32-ptr1-b-only', 'f32', 128, 192, 64, 0, 0, 0, 0, 0.5, -2.0, 'c', 'ptr1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f64-ptr1-b-only', 'f64', 128, 192, 64, 0, 0, 0, 0, -2.0, 0.0, 'c', 'ptr1', (64, 64, 1, 64, 0, 0, 0, 6, 1)),
    C('f32-bcast-a2d', 'f32', 128, 192, 64, 3, 0, 0, 0, -2.0, 1.0, '2d:c', 'c', (64, 64, 1, 64, 1, 0, 0, 6, 3)),
    C('f64-bcast-a2d', 'f64', 128, 192, 64, 3, 0, 0, 0, -2.0, -2.0, '2d:c', 'c', (64, 64, 1, 64, 1, 0, 0, 6, 3)),
    C('f32-bcast-b2d', 'f32', 128, 192, 64, 3, 0, 1, 0, 1.0, 0.0, 'c', '2d:win', (64, 64, 1, 64, 1, 0, 0, 6, 3)),
    C('f64-bcast-b2d', 'f64', 128, 192, 64, 3, 0, 1, 0, 1.0, 1.0, 'c', '2d:win', (64, 64, 1, 64, 1, 0, 0, 6, 3)),
    C('f32-bcast-a2d-tri', 'f32', 192, 200, 192, 3, 0, 0, AL, 1.0, -2.0, '2d:c', 'c', (64, 64, 1, 192, 0, 0, 1, 12, 3)),
    C('f64-bcast-a2d-tri', 'f64', 192, 200, 192, 3, 0, 0, AL, -1.0, 0.0, '2d:c', 'c', (64, 64, 1, 192, 0, 0, 1, 12, 3)),
    C('f32-expand-a', 'f32', 128, 192, 64, 3, 0, 0, 0, -1.0, 1.0, 'exp:c', 'c', (64, 64, 1, 64, 1, 0, 0, 6, 3)),
    C('f64-expand-a', 'f64', 128, 192, 64, 3, 0, 0, 0, -1.0, -2.0, 'exp:c', 'c', (64, 64, 1, 64, 1, 0, 0, 6, 3)),
    C('f32-expand-b', 'f32', 128, 192, 64, 3, 1, 0, 0, 0.5, 0.0, 'c', 'exp:ptr1', (64, 64, 1, 64, 0, 0, 0, 6, 3)),
    C('f64-expand-b', 'f64', 128, 192, 64, 3, 1, 0, 0, 0.5, 1.0, 'c', 'exp:ptr1', (64, 64, 1, 64, 0, 0, 0, 6, 3)),
    C('f32-copied-nc', 'f32', 128, 192, 64, 0, 0, 0, 0, 0.5, -2.0, 'nc', 'nc', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f64-copied-nc', 'f64', 128, 192, 64, 0, 0, 0, 0, -2.0, 0.0, 'nc', 'nc', (64, 64, 1, 64, 1, 0, 0, 6, 1)),
    C('f32-copied-nc-3d', 'f32', 100, 70, 30, 2, 1, 0, 0, -2.0, 1.0, 'nc', 'c', (64, 64, 1, 32, 0, 0, 0, 4, 2)),
    C('f64-copied-nc-3d', 'f64', 100, 70, 30, 2, 1, 0, 0, -2.0, -2.0, 'nc', 'c', (64, 64, 1, 32, 0, 0, 0, 4, 2)),
    C('f32-thin-b-col', 'f32', 130, 1, 70, 0, 0, 0, 0, 1.0, 0.0, 'c', 'thin', (64, 64, 1, 96, 0, 0, 0, 3, 1)),
    C('f64-thin-b-col', 'f64', 130, 1, 70, 0, 0, 0, 0, 1.0, 1.0, 'c', 'thin', (64, 64, 1, 96, 0, 0, 0, 3, 1)),
    C('f32-thin-a-row', 'f32', 1, 130, 70, 0, 0, 0, 0, 1.0, -2.0, 'thin', 'c', (64, 64, 1, 96, 0, 0, 0, 3, 1)),
    C('f64-thin-a-row', 'f64', 1, 130, 70, 0, 0, 0, 0, -1.0, 0.0, 'thin', 'c', (64, 64, 1, 96, 0, 0, 0, 3, 1)),
    C('f32-thin-a-col-t', 'f32', 1, 130, 70, 0, 1, 0, 0, -1.0, 1.0, 'thin', 'c', (64, 64, 1, 96, 0, 0, 0, 3, 1)),
    C('f64-thin-a-col-t', 'f64', 1, 130, 70, 0, 1, 0, 0, -1.0, -2.0, 'thin', 'c', (64, 64, 1, 96, 0, 0, 0, 3, 1)),
    C('f32-thin-b-row-t', 'f32', 130, 1, 70, 0, 0, 1, 0, 0.5, 0.0, 'c', 'thin', (64, 64, 1, 96, 0, 0, 0, 3, 1)),
    C('f64-thin-b-row-t', 'f64', 130, 1, 70, 0, 0, 1, 0, 0.5, 1.0, 'c', 'thin', (64, 64, 1, 96, 0, 0, 0, 3, 1)),
    C('f32-splitk-batched-beta', 'f32', 128, 192, 4096, 3, 0, 1, 0, 0.5, -2.0, 'c', 'c', (64, 64, 16, 256, 1, 1, 0, 6, 48)),
    C('f64-splitk-batched-beta', 'f64', 128, 192, 4096, 3, 0, 1, 0, 0.5, -2.0, 'c', 'c', (64, 64, 16, 256, 1, 1, 0, 6, 48)),
]
# GEMM_CASES_END


def plan_key(dt, plan):
    """What distinguishes one code path of a launch from another: (dtype, tile shape, whole, split-K, xcd_chunk, batch_perm)."""
    return (dt, plan[0], plan[1], plan[4], int(plan[2] > 1), plan[5], plan[6])


def operand_view(spec, val):
    """Store the dense tensor `val` ((batch,) R, C) the way `spec` says and return that view; everything of the parent
    buffer outside the view is NaN, so a read outside the operand shows in the result.
      c     contiguous
      win   a row-strided window of a larger matrix (rows 1.., columns 4..: vector loads stay possible when C % 4 == 0)
      ptr1  X[:, 1:C+1] of a row length C + 4: the base pointer is one element off, the strides are unchanged
      row1  X[1:, :]: the base pointer is one row (C elements) off
      tcol  a column-major window (the transpose of a window of a (C, R + 3) matrix)
      nc    X[::2, ::2]: neither stride is 1, `_mat_view` has to copy
      thin  R == 1 or C == 1 with a non-unit stride along the length-1 dimension (the stride rewrite of `_mat_view`)
    prefixes: `2d:` a 2-D operand against a batched one, `exp:` one matrix `expand`ed over the batch (batch stride 0)."""
    kind = spec.split(':')[-1]
    pre = spec.split(':')[0] if ':' in spec else ''
    if pre:
        val = val[0]
    R, Cc = val.shape[-2:]
    lead = tuple(val.shape[:-2])

    def parent(r, c):
        return torch.full(lead + (r, c), float('nan'), dtype=val.dtype, device=val.device)
    if kind == 'c':
        v = parent(R, Cc)
    elif kind == 'win':
        v = parent(R + 2, Cc + 8)[..., 1:R + 1, 4:Cc + 4]
    elif kind == 'ptr1':
        v = parent(R, Cc + 4)[..., :, 1:Cc + 1]
    elif kind == 'row1':
        v = parent(R + 1, Cc)[..., 1:, :]
    elif kind == 'tcol':
        v = parent(Cc, R + 3)[..., :, 1:R + 1].transpose(-1, -2)
    elif kind == 'nc':
        v = parent(2 * R, 2 * Cc)[..., ::2, ::2]
    elif kind == 'thin':
        assert R == 1 or Cc == 1
        v = parent(R, 6)[..., :, 1:4:3] if Cc == 1 else parent(6, 2 * Cc)[..., 1:4:3, ::2]
    else:
        raise ValueError(spec)
    assert tuple(v.shape) == tuple(val.shape)
    v.copy_(val)
    return v


def stored_shapes(case):
    """Shapes of A and B as stored (before op()), with the batch dimension the row asks for."""
    a = (case.K, case.M) if case.ta else (case.M, case.K)
    b = (case.N, case.K) if case.tb else (case.K, case.N)
    lead = (case.nb,) if case.nb else ()
    return lead + a, lead + b


def build_operands(case, device, fill=None):
    """(A, B) as the row stores them.  fill(shape, which) -> dense tensor of the stored shape (default: uninitialised)."""
    dt = DTYPES[case.dt]
    sa, sb = stored_shapes(case)
    if fill is None:
        fill = lambda shape, which: torch.zeros(shape, dtype=dt, device=device)   # noqa: E731
    A = operand_view(case.va, fill(sa, 'A'))
    B = operand_view(case.vb, fill(sb, 'B'))
    if case.va.startswith('exp:'):
        A = A.unsqueeze(0).expand(case.nb, *A.shape)
    if case.vb.startswith('exp:'):
        B = B.unsqueeze(0).expand(case.nb, *B.shape)
    return A, B


def query_plan(case):
    """The plan the C ABI reports for a row (no GPU): through ops.gemm_plan on CPU twins of the operands, or, for the
    two-level batch rows (contiguous diagonal blocks: vector loads on both sides), through nsgp_gemm_plan itself."""
    from nsgp import ops
    import nsgp
    if case.nb2 > 1:
        buf = (ctypes.c_int32 * 11)()
        rc = nsgp.load_library().nsgp_gemm_plan(case.M, case.N, case.K, case.nb, case.nb2, 4 if case.dt == 'f32' else 8,
                                                case.flags, 1, 1, 0, 1, ctypes.cast(buf, ctypes.c_void_p))
        assert rc == 0
        return tuple(buf)[:9]
    A, B = build_operands(case, 'cpu')
    return tuple(ops.gemm_plan(A, B, case.ta, case.tb, case.flags))[:9]


def reachable_keys():
    """Every plan key the planner produces over a coarse grid of shapes, batches, flags and load forms."""
    import nsgp
    lib = nsgp.load_library()
    buf = (ctypes.c_int32 * 11)()
    out = ctypes.cast(buf, ctypes.c_void_p)
    keys = {}
    sizes = (1, 64, 200, 256, 1024, 2048, 4096)
    flagsets = (0, AL, AU, BL, BU, CL, AL | BU | CL | NF, AL | BL | CL | NF, AU | BL)
    for dt, es in (('f32', 4), ('f64', 8)):
        for M, N, K, nb, fl, ns, vec in itertools.product(sizes, sizes, (16, 130, 512, 1024, 4096), (1, 2, 3), flagsets,
                                                          (0, NS), (0, 1)):
            assert lib.nsgp_gemm_plan(M, N, K, nb, 1, es, fl | ns, vec, vec, 0, 1, out) == 0
            keys.setdefault(plan_key(dt, tuple(buf)), (M, N, K, nb, fl | ns, vec))
    return keys


def test_case_names_are_unique_and_coefficients_come_from_the_stated_sets():
    names = [c.name for c in GEMM_CASES]
    assert len(set(names)) == len(names)
    for c in GEMM_CASES:
        assert c.alpha in ALPHAS and c.beta in BETAS and c.dt in DTYPES, c.name
        assert not (c.flags & AL and c.flags & AU) and not (c.flags & BL and c.flags & BU), c.name


def test_every_case_keeps_integer_arithmetic_exact():
    for c in GEMM_CASES:
        assert 4 * (32 * c.K + 16) < 2 ** 24, c.name


@pytest.mark.parametrize('case', GEMM_CASES, ids=lambda c: c.name)
def test_every_case_lands_on_its_expected_plan(case):
    assert query_plan(case) == case.plan, (case.name, plan_key(case.dt, query_plan(case)))


def test_the_table_reaches_every_reachable_plan():
    have = {plan_key(c.dt, c.plan) for c in GEMM_CASES}
    want = reachable_keys()
    missing = {k: v for k, v in want.items() if k not in have}
    assert not missing, f'plan keys no row of GEMM_CASES runs (key: first (M, N, K, nb, flags, vec) that gives it): {missing}'


def test_the_table_covers_the_layouts_flags_and_production_shapes_by_name():
    rows = GEMM_CASES
    # all four (modeA, modeB) layouts with and without vector loads, per tile shape and dtype
    for dt, tile in (('f32', (64, 64)), ('f64', (64, 64)), ('f32', (128, 128)), ('f32', (128, 64))):
        for ta, tb, whole in itertools.product((False, True), (False, True), (0, 1)):
            assert any(c.dt == dt and c.plan[:2] == tile and c.ta == ta and c.tb == tb and c.plan[4] == whole and
                       c.va in ('c', 'ptr1') and c.vb == c.va and c.M % c.plan[0] == 0 and c.N % c.plan[1] == 0 and c.K % 32 == 0
                       for c in rows), (dt, tile, ta, tb, whole)
    # every triangle flag alone, in a split and in a single-pass launch
    for f in (AL, AU, BL, BU, CL):
        for split in (False, True):
            assert any(c.flags & ~NS == f and (c.plan[2] > 1) == split for c in rows), (f, split)
    # the combined products of the Cholesky adjoint, the halved diagonal with and without split-K
    for f in (AL | BU | CL | NF | HD, AL | BL | CL | NF, AU | BL, AL | BU):
        assert any(c.flags & ~NS == f for c in rows), f
    for split in (False, True):
        assert any(c.flags & HD and (c.plan[2] > 1) == split for c in rows), split
    assert any(c.flags & CL and c.M > c.N for c in rows) and any(c.flags & CL and c.M < c.N for c in rows)
    assert any(c.flags & CL and c.beta != 0 and c.plan[2] == 1 for c in rows)
    assert any(c.flags & CL and c.beta != 0 and c.plan[2] > 1 for c in rows)
    # production shapes
    for N in (4096, 5120):
        for ns in (0, NS):
            assert any((c.M, c.N, c.K) == (1024, N, 1024) and c.flags in (AL | ns, AU | ns) for c in rows), (N, ns)
    assert any((c.M, c.N, c.K, c.flags) == (1024, 4096, 1024, AU) and c.ta for c in rows)           # Kzxbar = W^T Abar
    assert any((c.M, c.N, c.K) == (1024, 1024, 4096) and c.flags & CL and c.tb for c in rows)       # Wbar = tril(Abar Kzx^T)
    assert sum((c.M, c.N, c.K, c.nb) == (1024, 1024, 1024, 3) for c in rows) >= 6                   # the 3 x 1024^2 adjoint
    assert any(c.N == 1 for c in rows)
    assert any(c.nb2 > 1 for c in rows)


def test_plan_query_rejects_bad_arguments_and_reports_empty_launches():
    import nsgp
    lib = nsgp.load_library()
    buf = (ctypes.c_int32 * 11)()
    out = ctypes.cast(buf, ctypes.c_void_p)
    ok = [64, 64, 16, 1, 1, 4, 0, 1, 1, 0, 1, out]
    bad = lambda i, v: lib.nsgp_gemm_plan(*[v if k == i else a for k, a in enumerate(ok)])   # noqa: E731
    assert bad(0, -1) == -1 and bad(1, -1) == -2 and bad(2, -1) == -3 and bad(3, 0) == -4 and bad(4, 0) == -5
    assert bad(5, 2) == -6 and bad(6, AL | AU) == -7 and bad(6, BL | BU) == -7
    assert bad(9, 2) == -10 and bad(10, -1) == -11 and bad(11, None) == -12
    assert bad(0, 0) == 0 and tuple(buf) == (0,) * 11
    assert bad(2, 0) == 0 and tuple(buf)[:9] == (64, 64, 1, 32, 1, 0, 0, 1, 1)
    # the split reported here is the split nsgp_gemm_workspace sizes
    for M, N, K, nb, fl in ((1024, 1024, 40960, 1, CL), (1024, 40960, 1024, 1, 0), (128, 192, 4096, 3, 0)):
        assert lib.nsgp_gemm_plan(M, N, K, nb, 1, 4, fl, 1, 1, 0, 1, out) == 0
        assert lib.nsgp_gemm_workspace(M, N, K, nb, 1, 4, fl) == (buf[2] * nb * M * N * 4 if buf[2] > 1 else 0)
