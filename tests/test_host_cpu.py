"""CPU-only checks of the host side: the C-ABI library loads and exports every symbol the header
declares, the nn.Module mirrors have the reference's state_dict layout, data containers behave,
the product refuses to run without a GPU (no CPU fallback), and the batch-sharded gradient
all-reduce is equivalent to one big batch (gloo, world_size 2)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from crfconv_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'crfconv_amd.h')).read()
    declared = set(re.findall(r'\b(crfconv_[a-z0-9_]+)\s*\(', header))
    assert declared, 'no declarations parsed'
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.crfconv_abi_version() == 1
    # argument validation happens before any HIP call, so it is testable without a GPU
    rc = lib.crfconv_meanfield_forward(None, None, None, 16, 1, 10, 7, None, None, 1, None, None, None)
    assert rc == -3
    rc = lib.crfconv_meanfield_forward_u16(None, None, None, None, 1, 1, 16, 1, 10, 7, None, None, 1, None, None, None)
    assert rc == -3 and b'H=7' in lib.crfconv_last_error()
    rc = lib.crfconv_knn_batch_dev(None, 1, 10, 3, None, 10, 4, None, None, None, 0, None)
    assert rc == -1


def test_meanfield_width_list_has_no_default_case():
    """One list of hidden widths behind the mean-field entries (csrc/crf_common.hpp CRF_WIDTHS): a width outside it is refused or
    answered with 0, never treated as 64."""
    from crfconv_amd import _lib
    lib = _lib.load()
    for H in (4, 8, 16, 32, 64):
        assert lib.crfconv_meanfield_backward_supported(H, 16, 1) == 1 and lib.crfconv_meanfield_backward_supported(H, 32, 1) == 1
        assert lib.crfconv_meanfield_backward_supported(H, 16, 0) == 0 and lib.crfconv_meanfield_backward_supported(H, 9, 1) == 0
        assert lib.crfconv_meanfield_backward_workspace(1000, H, 16) > 0
    for H in (0, 7, 12, 65, 128):
        assert lib.crfconv_meanfield_backward_supported(H, 16, 1) == 0
        assert lib.crfconv_meanfield_backward_workspace(1000, H, 16) == 0
        assert lib.crfconv_meanfield_step(None, None, None, None, 16, 1, 10, H, None, None, None, None) == -3
        assert lib.crfconv_meanfield_bwd_edge(None, None, None, None, 16, 1, 10, H, None, None, None, None, 0, None) == -3
        assert lib.crfconv_similarity_bwd(None, None, None, None, 16, 1, 10, H, None, None, None) == -3
        assert (b'H=%d' % H) in lib.crfconv_last_error()
    assert lib.crfconv_wide_similarity(None, None, 16, 0, 10, 64, None, None) == -3
    assert lib.crfconv_wide_similarity(None, None, 16, 0, 10, 128, None, None) == -1      # a wide width: on to the null-pointer check


def test_kernel_weights_entries_check_their_arguments():
    """crfconv_kernel_weights_forward / _backward (csrc/discrete.hip) refuse before any HIP call: row and degree range (-1), kernel count
    and hidden width outside what is compiled (-3), null pointers and dfk aliasing dfk_self (-1); the float64 dW partials are one slab of
    DW_GMAX = 8 per workgroup of DW_ROWS = 4 rows."""
    from crfconv_amd import _lib
    lib = _lib.load()

    def fwd(K=16, G=5, H=64, m=10, p=None):
        return lib.crfconv_kernel_weights_forward(p, p, K, p, G, H, m, p, None)

    def bwd(K=16, G=5, H=64, m=10, p=None, dfk=None):
        return lib.crfconv_kernel_weights_backward(p, p, p, p, p, K, p, G, H, m, p, p if dfk is None else dfk, p, None)

    for f in (fwd, bwd):
        assert f() == -1 and b'null pointer' in lib.crfconv_last_error()
        for G in (0, 9):
            assert f(G=G) == -3 and (b'num_kernels=%d' % G) in lib.crfconv_last_error()
        for H in (0, 257):
            assert f(H=H) == -3 and (b'hidden_channels=%d' % H) in lib.crfconv_last_error()
        for K in (0, 65):
            assert f(K=K) == -1 and (b'K=%d' % K) in lib.crfconv_last_error()
        for m in (0, -1):
            assert f(m=m) == -1 and b'out of range' in lib.crfconv_last_error()
        assert f(K=64, m=2 ** 31 // 64) == -1 and b'out of range' in lib.crfconv_last_error()       # m * K == 2^31: edge ids leave int32
        assert f(K=64, m=2 ** 31 // 64 - 1) == -1 and b'null pointer' in lib.crfconv_last_error()   # the largest table passes the range check
        for G, H, K in ((1, 1, 1), (8, 256, 64)):                                                   # the corners of what is compiled
            assert f(G=G, H=H, K=K) == -1 and b'null pointer' in lib.crfconv_last_error()
    # never dereferenced: the alias check refuses in front of the first launch
    import ctypes
    a, b = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    pa, pb = ctypes.addressof(a), ctypes.addressof(b)
    assert bwd(p=pa) == -1 and b'alias' in lib.crfconv_last_error()
    assert bwd(p=pa, dfk=pb, G=9) == -3
    assert [lib.crfconv_kernel_weights_partials(m) for m in (1, 4, 5)] == [8, 8, 16]


def test_meanfield_backward_entry_checks_its_arguments():
    """crfconv_meanfield_backward (csrc/crf_bwd.hip) refuses before any HIP call -- every call here is refused, none launches: T = 0 and
    shapes outside the fast ones (-3), the operands of the width's dP / dQ form missing (H = 8 / 16: dP, dQ and the ticket; other widths:
    mts and sumG), a workspace one byte short or not 16-byte aligned (-1).  The workspace grows by one dP and one dQ slab of H x H
    floats where the edge pass gains a workgroup (Geo<H>::PPB = 64 / (H / 4) x 4 rows each)."""
    import ctypes
    from crfconv_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15                 # never dereferenced

    def bwd(H=8, K=16, k0=1, m=10, T=2, mts=p, sumG=p, dP=p, dQ=p, ticket=p, ws=p, short=0, first=p):
        need = lib.crfconv_meanfield_backward_workspace(m, H, K)
        return lib.crfconv_meanfield_backward(first, p, p, p, p, p, None, 1, 1, p, p, K, k0, m, H, p, p, T, p, p, mts, sumG, p, p, p, p, dP, dQ,
                                              ws, need - short, ticket, None)

    for H in (4, 8, 16, 32, 64):
        assert bwd(H=H, T=0) == -3 and b'T=0' in lib.crfconv_last_error()
        assert bwd(H=H, K=16, k0=0) == -3 and bwd(H=H, K=9) == -3 and bwd(H=H, K=64) == -3
        assert bwd(H=H, K=65) == -1 and bwd(H=H, m=0) == -1
        assert bwd(H=H, first=None) == -1 and b'null pointer' in lib.crfconv_last_error()
        assert bwd(H=H, ws=None) == -1 and b'null pointer' in lib.crfconv_last_error()
        inside = lib.crfconv_meanfield_backward_param_grads_inside(H) == 1
        assert inside == (H in (8, 16))
        for missing in ((dict(dP=None), dict(dQ=None), dict(ticket=None)) if inside else (dict(mts=None), dict(sumG=None))):
            assert bwd(H=H, **missing) == -1 and b'required' in lib.crfconv_last_error()
        # what the other form takes may be absent: the call gets as far as the workspace check
        other = dict(mts=None, sumG=None) if inside else dict(dP=None, dQ=None, ticket=None)
        assert bwd(H=H, short=1, **other) == -1 and b'workspace' in lib.crfconv_last_error()
        assert bwd(H=H, short=1) == -1 and b'workspace' in lib.crfconv_last_error()
        assert bwd(H=H, ws=p + 4) == -1 and b'workspace' in lib.crfconv_last_error()
        assert bwd(H=H, ws=p + 8, K=32) == -1 and b'workspace' in lib.crfconv_last_error()
    assert bwd(H=12) == -3 and b'H=12' in lib.crfconv_last_error()
    for H in (8, 16, 32, 64):                               # (H = 4: a slab of 64 bytes disappears in the 256-byte rounding)
        ppb = 64 // (H // 4) * 4
        ws = lambda m: lib.crfconv_meanfield_backward_workspace(m, H, 16)
        for blocks in (1, 127, 128):
            m0 = blocks * ppb                               # even: m0 x 16 records of 8 bytes are whole 256-byte units
            assert ws(m0) - ws(m0 - 2) == 256 and ws(m0 + 2) - ws(m0) == 256 + 2 * H * H * 4, (H, blocks)


def test_wide_meanfield_entries_check_their_arguments():
    """The five crfconv_wide_* entries (csrc/crf_wide.hip) refuse before any HIP call: K = 65, k0 = K, m = 0 and null pointers (-1), an
    output aliasing its input (aggregate: out == x; scatter: out == src; similarity_bwd: w == ds) (-1), H = 64 (-3)."""
    import ctypes
    from crfconv_amd import _lib
    lib = _lib.load()
    a, b = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    p, o = ctypes.addressof(a), ctypes.addressof(b)        # never dereferenced
    entries = dict(
        similarity=lambda K=16, k0=0, m=10, H=128, p=p, out=o: lib.crfconv_wide_similarity(p, p, K, k0, m, H, out, None),
        aggregate=lambda K=16, k0=0, m=10, H=128, p=p, out=o: lib.crfconv_wide_aggregate(p, p, p, K, k0, m, H, out, None),
        bwd_edge=lambda K=16, k0=0, m=10, H=128, p=p, out=o: lib.crfconv_wide_bwd_edge(p, p, p, K, k0, m, H, out, 0, None),
        scatter=lambda K=16, k0=0, m=10, H=128, p=p, out=o: lib.crfconv_wide_scatter(p, p, p, p, K, m, H, None, 0, out, None),
        similarity_bwd=lambda K=16, k0=0, m=10, H=128, p=p, out=o: lib.crfconv_wide_similarity_bwd(p, p, p, p, K, k0, m, H, out, o, None))
    for name, f in entries.items():
        for H in (128, 256):
            assert f(H=H, K=65) == -1 and b'K=65' in lib.crfconv_last_error(), name
            assert f(H=H, K=0) == -1 and f(H=H, m=0) == -1, name
            if name != 'scatter':                           # (the scatter walks the reverse list: it has no k0)
                assert f(H=H, k0=16) == -1 and b'k0=16' in lib.crfconv_last_error(), name
                assert f(H=H, K=64, k0=64) == -1, name
            assert f(H=H, p=None) == -1 and b'null pointer' in lib.crfconv_last_error(), name
            assert f(H=H, out=None) == -1 and b'null pointer' in lib.crfconv_last_error(), name
            assert f(H=H, K=64, k0=0, p=None) == -1 and b'null pointer' in lib.crfconv_last_error(), name      # the corner of what is compiled
        for H in (64, 0, 129, 512):
            assert f(H=H) == -3 and (b'got %d' % H) in lib.crfconv_last_error(), name
    for name in ('aggregate', 'scatter', 'similarity_bwd'):          # out == x, out == src, w == ds
        assert entries[name](out=p) == -1 and b'alias' in lib.crfconv_last_error(), name


def test_pointconv_entries_check_their_arguments():
    """The crfconv_pointconv_* entries (csrc/pointconv.hip, pointconv_bwd.hip, pointconv_fold.hip, pointconv_wide_params.hip) refuse before
    any HIP call: K = 0 and K = 65 (-1), m = 0 (-1), a width outside {4, 8, 16, 32, 64, 128} (-3, "unsupported"), null pointers (-1), a
    workspace that is too small (-4: forward_uv, bwd_reduce, bwd_params, bwd_input_reduce, bwd_a1, moments_packed), bwd_input_reduce
    without a ticket, combine with one running tensor of the pair, bwd_params beyond d = 16 and with one output of the pair,
    forward_uv_hosting at a non-hosting width; wide_params_supported / wide_params_nblk outside the matrix-pipe pass."""
    import ctypes
    from crfconv_amd import _lib
    lib = _lib.load()
    a = ctypes.create_string_buffer(64)
    p = ctypes.addressof(a)                                  # never dereferenced
    big = 1 << 30
    err = lib.crfconv_last_error
    E = dict(
        forward=lambda K=16, m=10, d=8, p=p, o=p: lib.crfconv_pointconv_forward(p, p, p, p, K, m, d, p, p, p, 0.1, p, p, o, None),
        forward_uv=lambda K=16, m=10, d=8, p=p, o=p, ws=big: lib.crfconv_pointconv_forward_uv(p, p, p, p, K, m, d, p, p, p, 0.1, p, p, p, p, o, p, ws, p, None),
        bwd_input=lambda K=16, m=10, d=8, p=p, o=p: lib.crfconv_pointconv_bwd_input(p, p, p, p, p, K, m, d, p, p, p, 0.1, p, p, o, None),
        bwd_input_reduce=lambda K=16, m=10, d=8, p=p, o=p, ws=big, tk=p, mt=10: lib.crfconv_pointconv_bwd_input_reduce(
            p, p, p, p, p, K, m, mt, d, p, p, p, 0.1, p, p, o, p, p, p, p, p, 160.0, 1, p, p, p, p, p, p, ws, tk, None),
        bwd_reduce=lambda K=16, m=10, d=8, p=p, o=p, ws=big: lib.crfconv_pointconv_bwd_reduce(p, p, p, p, p, K, m, d, p, p, p, 0.1, p, o, p, ws, None),
        bwd_params=lambda K=16, m=10, d=8, p=p, o=p, ws=big, o1=p, o2=p: lib.crfconv_pointconv_bwd_params(p, p, p, p, p, K, m, d, p, p, p, 0.1, p, p, p, o1, o2,
                                                                                                       o, ws, None),      # (o: the workspace)
        bwd_dump=lambda K=16, m=10, d=32, p=p, o=p: lib.crfconv_pointconv_bwd_dump(p, p, p, p, p, K, m, d, p, p, p, 0.1, p, p, p, p, p, o, None),
        moments_packed=lambda K=16, m=10, d=4, p=p, o=p, ws=big, n=160.0: lib.crfconv_pointconv_moments_packed(p, p, p, K, m, n, p, p, p, o, p, ws, None))
    for name, f in E.items():
        assert f(K=0) == -1 and b'K=0' in err(), name
        assert f(K=65) == -1 and b'K=65' in err(), name
        assert f(K=64, m=0) == -1 and b'rows=0' in err(), name
        assert f(m=1 << 31) == -1, name
        assert f(p=None) == -1 and b'null pointer' in err(), name
        assert f(o=None) == -1 and b'null pointer' in err(), name
        assert f(K=1, m=1, p=None) == -1 and f(K=64, o=None) == -1, name          # the corners of what is accepted
        if name != 'moments_packed':                                                # (the moments have no width)
            for d in (0, 2, 12, 24, 48, 96, 256):
                assert f(d=d) == -3 and (b'd=%d' % d) in err(), (name, d)
        if name != 'bwd_dump':
            for d in ((4, 8, 16) if name == 'bwd_params' else (4, 8, 16, 32, 64, 128)):
                assert f(d=d, K=65) == -1 and f(d=d, p=None) == -1, (name, d)
    for name in ('forward_uv', 'bwd_reduce', 'bwd_params', 'bwd_input_reduce', 'moments_packed'):
        for d in ((4, 16) if name in ('bwd_params', 'moments_packed') else (4, 32, 128)):      # (d = 32, 128 at K = 16: the matrix-pipe branch of forward_uv)
            assert E[name](d=d, ws=0) == -4 and b'workspace too small' in err(), (name, d)
            assert E[name](d=d, ws=7, m=5000) == -4, (name, d)
    assert E['bwd_input_reduce'](tk=None) == -1 and b'null pointer' in err()
    assert E['bwd_input_reduce'](mt=0) == -1 and b'rows=0' in err()                  # the target count is checked on its own
    assert E['bwd_params'](d=32) == -3 and b'd <= 16' in err()
    assert E['bwd_params'](o1=None) == -1 and E['bwd_params'](o2=None) == -1 and b'both or neither' in err()
    assert E['moments_packed'](n=0.0) == -1 and b'n_edges' in err()
    assert E['bwd_dump'](K=64, m=1 << 25) == -1 and b'too many edges' in err()

    def combine(m=10, d=8, p=p, o=p, rm=p, rv=p):
        return lib.crfconv_pointconv_combine(p, p, p, p, p, p, 160.0, rm, rv, 0.1, 1e-5, m, d, p, p, p, o, None)
    assert combine(rm=None) == -1 and b'pair' in err() and combine(rv=None) == -1 and b'pair' in err()
    assert combine(m=0) == -1 and combine(d=12) == -3 and combine(p=None) == -1 and combine(o=None) == -1 and b'null pointer' in err()

    def a1(n=160, d=32, p=p, o=p, ws=big):
        return lib.crfconv_pointconv_bwd_a1(p, p, p, n, d, 0.1, o, p, ws, None)
    assert a1(p=None) == -1 and b'null pointer' in err()
    assert a1(n=0) == -1 and a1(n=1 << 31) == -1 and b'n_edges' in err()
    for d in (4, 12, 256):                                   # (d = 4 has no dump path)
        assert a1(d=d) == -3 and (b'd=%d' % d) in err()
    for d in (8, 16, 32, 64, 128):
        assert a1(d=d, ws=0) == -4 and a1(d=d, ws=lib.crfconv_pointconv_bwd_a1_workspace(160, d) - 1) == -4 and b'workspace too small' in err()

    def hosting(K=16, m=10, d=8, p=p, n=1):
        return lib.crfconv_pointconv_forward_uv_hosting(p, p, p, p, K, m, d, p, p, p, 0.1, p, p, p, p, p, p, big, p, p, p, n, p, p, None)
    for d in (4, 16, 32, 64, 128):
        assert lib.crfconv_pointconv_forward_uv_hosts(16, d) == 0 and hosting(d=d) == -3 and b'not a hosting width' in err(), d
    assert lib.crfconv_pointconv_forward_uv_hosts(16, 8) == 1 and lib.crfconv_pointconv_forward_uv_hosts(5, 8) == 1
    assert hosting(K=65) == -1 and hosting(m=0) == -1 and hosting(p=None) == -1 and hosting(n=0) == -1 and b'n=0' in err()

    for d in (32, 64, 128):
        assert lib.crfconv_pointconv_wide_params_supported(640, 16, d) == 1 and lib.crfconv_pointconv_wide_params_nblk(640, d) > 0
        for K in (1, 4, 15, 17, 32, 64):
            assert lib.crfconv_pointconv_wide_params_supported(640, K, d) == 0, (K, d)
        assert lib.crfconv_pointconv_wide_params_supported(0, 16, d) == 0 and lib.crfconv_pointconv_wide_params_supported(1 << 27, 16, d) == 0
        assert lib.crfconv_pointconv_wide_params_nblk(0, d) == 0 and lib.crfconv_pointconv_wide_params_nblk(-5, d) == 0
    for d in (4, 8, 16, 48, 256):
        assert lib.crfconv_pointconv_wide_params_supported(640, 16, d) == 0, d
    job = _lib.PcWideJob(p, p, p, p, p, 5, 640, 32, p, p, p, 0.1, p, p, p, p, p)        # K = 5: the jobs entry refuses what `supported` does
    assert lib.crfconv_pointconv_wide_params_jobs((_lib.PcWideJob * 1)(job), 1, None) == -3 and b'K=5' in err()


def test_streaming_mlp_entries_check_their_arguments():
    """The entries of the row-streaming dense stack (csrc/linear.hip, mlp_bwd.hip, bn_records.hip, wgrad.hip) refuse before any HIP call
    -- every call here is refused, none launches: null pointers (-1), M <= 0 (-1; the fused backward answers through its `supported`
    query: -3), a width whose weight slab does not fit LDS (-3), a split that is not a multiple of 4 or lies outside (0, Ci) (-1), a
    dropout probability outside [0, 1) (-1), Co % 4 != 0 where the entry needs it (-3), a workspace one byte short (-4), more than BA_MAX = 4
    jobs (-1).  The `_supported` and `_workspace` queries answer 0 for non-positive shapes."""
    import ctypes
    from crfconv_amd import _lib
    lib = _lib.load()
    a = ctypes.create_string_buffer(1024)
    p = (ctypes.addressof(a) + 255) & ~255                   # never dereferenced; 256-byte aligned for the partial pass
    err = lib.crfconv_last_error
    big = 1 << 40

    # ---- the forward entries: (X, W, Y) null, M, the slab, the split, p, Co % 4
    def fwd(M=10, Ci=16, Co=16, x=p, w=p, y=p):
        return lib.crfconv_linear_forward(x, w, p, M, Ci, Co, 0, y, p, None)

    def drop(M=10, Ci=16, Co=16, x=p, w=p, y=p, prob=0.5, ctr=p):
        return lib.crfconv_linear_forward_dropout(x, w, M, Ci, Co, 1, prob, 7, ctr, y, None)

    def cat(M=10, Ci=16, Co=16, x=p, w=p, y=p, xb=p, split=8):
        return lib.crfconv_linear_forward_cat(x, xb, split, w, p, M, Ci, Co, y, p, None)

    def bna(M=10, Ci=16, Co=16, x=p, w=p, y=p, xb=None, split=0, coef=p):
        return lib.crfconv_linear_bn_act(x, xb, split, w, p, coef, p, 0.1, M, Ci, Co, y, None)
    for name, f in (('forward', fwd), ('dropout', drop), ('cat', cat), ('bn_act', bna)):
        for missing in (dict(x=None), dict(w=None), dict(y=None)):
            assert f(**missing) == -1 and b'null pointer' in err(), (name, missing)
        for M in (0, -3):
            assert f(M=M) == -1 and b'M must be positive' in err(), (name, M)
        for Ci, Co in ((1012, 16), (2048, 64), (0, 16), (16, 0), (-4, 16)):        # (1008 inputs are the last that fit beside 16 outputs)
            assert f(Ci=Ci, Co=Co) == -3 and b'does not fit LDS' in err(), (name, Ci, Co)
        assert f(Ci=1008, Co=16, x=None) == -1 and f(Ci=512, Co=1024, y=None) == -1 and b'null pointer' in err(), name
    assert drop(ctr=None) == -1 and b'null pointer' in err()
    for prob in (1.0, 1.5, -0.1):
        assert drop(prob=prob) == -1 and b'outside [0, 1)' in err(), prob
    assert cat(xb=None) == -1 and b'null pointer' in err()
    for Ci, split in ((16, 0), (16, 16), (16, 20), (16, -4), (16, 6), (30, 8), (18, 9)):
        assert cat(Ci=Ci, split=split) == -1 and b'two-operand form' in err(), (Ci, split)
        assert bna(Ci=Ci, split=split, xb=p) == -1 and b'two-operand form' in err(), (Ci, split)
    assert bna(coef=None) == -1 and b'null pointer' in err()
    for Co in (13, 18, 2):
        assert bna(Co=Co) == -3 and b'multiple of 4' in err(), Co
    for Ci, Co in ((0, 16), (16, 0), (-1, 16), (16, -1), (1012, 16)):
        assert lib.crfconv_linear_forward_supported(Ci, Co) == 0, (Ci, Co)
    assert lib.crfconv_linear_forward_supported(1008, 16) == 1 and lib.crfconv_linear_forward_supported(1, 1) == 1

    # ---- the fused backward: four entries over one implementation
    def ws_of(M, Ci, Co):
        return lib.crfconv_mlp_backward_workspace(M, Ci, Co)

    def plain(M=10, Ci=16, Co=16, q=p, dx=p, ws=p, short=0, **_):
        return lib.crfconv_mlp_backward(q, q, q, q, q, 0.1, M, Ci, Co, dx, p, p, p, ws, ws_of(M, Ci, Co) - short, p, None)

    def add(M=10, Ci=16, Co=16, q=p, dx=p, ws=p, short=0, extra=p):
        return lib.crfconv_mlp_backward_add(q, q, q, q, q, 0.1, M, Ci, Co, extra, dx, p, p, p, ws, ws_of(M, Ci, Co) - short, p, None)

    def masked(M=10, Ci=16, Co=16, q=p, dx=p, ws=p, short=0, extra=p):
        return lib.crfconv_mlp_backward_add_mask(q, q, q, q, q, 0.1, M, Ci, Co, extra, 0.1, dx, p, p, p, ws, ws_of(M, Ci, Co) - short, p, None)

    def cat_bwd(M=10, Ci=16, Co=16, q=p, dx=p, ws=p, short=0, xb=p, split=8, dxb=p):
        return lib.crfconv_mlp_backward_cat(q, q, q, xb, split, q, q, 0.1, M, Ci, Co, dx, dxb, p, p, p, ws, ws_of(M, Ci, Co) - short, p, None)
    for name, f in (('plain', plain), ('add', add), ('masked', masked), ('cat', cat_bwd)):
        assert f(q=None) == -1 and f(ws=None) == -1 and b'null pointer' in err(), name
        for M in (0, -2):
            assert f(M=M) == -3 and b'not supported' in err(), (name, M)
        for Ci, Co in ((16, 18), (16, 2)):                                      # Co % 4: the masked form says so itself
            assert f(Ci=Ci, Co=Co) == (-1 if name == 'masked' else -3), (name, Ci, Co)
            assert (b'multiples of 4' if name == 'masked' else b'not supported') in err(), (name, Ci, Co)
        for Ci, Co in ((16, 0), (16, 1028), (16, 784), (1028, 16)):      # Co < 4, the ranges, the dX slab of Co inputs (768 fit)
            assert f(Ci=Ci, Co=Co) == -3 and b'not supported' in err(), (name, Ci, Co)
        assert f(short=1) == -4 and b'workspace too small' in err(), name
        assert f(Ci=1008, Co=16, short=1) == -4 and f(Ci=16, Co=768, short=1) == -4, name                 # the corners of what is accepted
    assert add(dx=None) == -1 and b'dX_add without dX' in err()
    assert masked(dx=None) == -1 and b'masked form' in err()
    for Ci in (6, 18):
        assert masked(Ci=Ci) == -1 and b'masked form' in err(), Ci
    assert cat_bwd(xb=None) == -1 and b'two-operand form' in err()
    assert cat_bwd(dxb=None) == -1 and cat_bwd(dx=None) == -1 and b'both or neither' in err()
    for Ci, split in ((16, 0), (16, 16), (16, 20), (16, 6), (30, 8)):
        assert cat_bwd(Ci=Ci, split=split) == -1 and b'two-operand form' in err(), (Ci, split)
    for M, Ci, Co in ((0, 16, 16), (-1, 16, 16), (10, 0, 16), (10, 16, 0), (10, -8, 16), (10, 16, -8)):
        assert lib.crfconv_mlp_backward_supported(M, Ci, Co) == 0 and lib.crfconv_mlp_backward_workspace(M, Ci, Co) == 0, (M, Ci, Co)
        assert lib.crfconv_linear_wgrad_workspace(M, Co, Ci) == 0 and lib.crfconv_linear_wgrad_nblk(M, Co, Ci) == 0, (M, Ci, Co)
    assert lib.crfconv_mlp_backward_supported(10, 16, 768) == 1 and lib.crfconv_mlp_backward_supported(10, 1008, 16) == 1
    assert lib.crfconv_mlp_backward_supported(10, 6, 16) == 1 and ws_of(10, 16, 16) > 0

    # ---- BatchNorm from the records
    def coef(M=10, C=16, q=p, out=p):
        return lib.crfconv_bn_coef_from_records(q, M, C, q, q, p, p, 0.1, 1e-5, out, None)

    def apply(M=10, C=16, q=p, out=p, nrec=1):
        return lib.crfconv_bn_apply_from_records(q, nrec, q, M, C, q, q, p, p, 0.1, 1e-5, None, 0.1, out, out, None)
    for name, f in (('coef', coef), ('apply', apply)):
        assert f(q=None) == -1 and f(out=None) == -1 and b'null pointer' in err(), name
        for bad in (dict(M=0), dict(M=-1), dict(C=0), dict(C=-4)):
            assert f(**bad) == -1 and b'bad shape' in err(), (name, bad)
    for bad in (dict(C=2), dict(C=18), dict(nrec=0), dict(nrec=-1), dict(nrec=1 << 31)):
        assert apply(**bad) == -1 and b'bad shape' in err(), bad

    def jobs(n, M=10, C=16, q=p, nrec=1, arr=True):
        rec = (_lib.BnApplyJob * max(n, 1))(*[_lib.BnApplyJob(q, nrec, q, M, C, q, q, p, p, 0.1, 1e-5, None, 0.1, q, q) for _ in range(max(n, 1))])
        return lib.crfconv_bn_apply_from_records_jobs(rec if arr else None, n, None)
    for n in (0, -1, 5, 64):
        assert jobs(n) == -1 and (b'1 .. 4 jobs (got %d)' % n) in err(), n
    assert jobs(1, arr=False) == -1 and b'1 .. 4 jobs' in err()
    for n in (1, 4):
        assert jobs(n, q=None) == -1 and b'job 0: null pointer' in err(), n
        for bad in (dict(M=0), dict(C=0), dict(C=6), dict(nrec=0), dict(nrec=1 << 31)):
            assert jobs(n, **bad) == -1 and b'job 0: bad shape' in err(), (n, bad)

    # ---- the partial pass of the plain weight gradient
    def partial(M=10, Co=16, Ci=16, g=p, ws=p, short=0, nblk=p):
        return lib.crfconv_linear_wgrad_partial(g, g, M, Co, Ci, 1, ws, lib.crfconv_linear_wgrad_workspace(M, Co, Ci) - short if M > 0 and Co > 0 and Ci > 0 else big,
                                                nblk, None)
    assert partial(g=None) == -1 and partial(ws=None) == -1 and partial(nblk=None) == -1 and b'null pointer' in err()
    for bad in (dict(M=0), dict(M=-1), dict(Co=0), dict(Ci=0), dict(Co=4097), dict(Ci=4097)):
        assert partial(**bad) == -1 and b'bad shape' in err(), bad
    assert partial(ws=p + 16) == -1 and b'256-byte aligned' in err()
    assert partial(short=1) == -4 and b'workspace too small' in err()
    assert partial(Co=4096, Ci=4096, short=1) == -4 and partial(Co=5, Ci=7, short=1) == -4


def test_state_dict_layout_matches_reference(golden):
    from crfconv_amd import models
    g = golden('g5_pointconvbig.npz')
    for tagc, use_crf in (('crf', True), ('ups', False)):
        net = models.PointConvBig(6, 13, use_crf=use_crf, steps=3)
        sd = net.state_dict()
        want = {k: (tuple(int(s) for s in sh.split(',')) if sh else ()) for k, sh in zip(g[tagc + '/keys'], g[tagc + '/shapes'])}
        assert set(sd) == set(want)
        for k, shp in want.items():
            assert tuple(sd[k].shape) == shp, k
    assert sum(p.numel() for p in models.PointConvBig(6, 13, True, 3).parameters()) == 820141
    crf = models.ContinuousGaussianCRFConv(64, 32, 32, steps=3)
    assert torch.equal(crf.c.data, torch.eye(8))                     # identity init (reference :36)
    g1 = golden('g1_crfconv.npz')
    crf.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g1.items() if k.startswith('sd/')}, strict=True)


def test_no_cpu_fallback():
    from crfconv_amd import models
    from crfconv_amd._lib import CrfConvError
    m = models.ContinuousGaussianCRFConv(64, 32, 32, steps=1)
    with pytest.raises(CrfConvError, match='no CPU path'):
        m(torch.zeros(2, 8, 64), torch.zeros(2, 32, 32), torch.zeros(2, 32, 1, dtype=torch.long),
          torch.zeros(2, 32, 16, dtype=torch.long))


def test_product_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'crfconv_amd')):
        for f in files:
            if f.endswith(('.py', '.hip', '.hpp')):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, re.M), os.path.join(dirpath, f)
                assert '/root/reference' not in src, os.path.join(dirpath, f)


def test_data_containers():
    from crfconv_amd import Data, MultiScaleData
    d = MultiScaleData(x=torch.zeros(2, 4, 6), y=torch.ones(2, 4, dtype=torch.long),
                       multiscale=[Data(pos=torch.zeros(2, 4, 3), neighbor_idx=torch.zeros(2, 4, 2, dtype=torch.long))])
    e = d.to('cpu')
    assert e is not d and e.multiscale[0].pos.shape == (2, 4, 3) and 'x' in e.keys
    assert 'MultiScaleData' in repr(e)


def test_mlp_refuses_cpu_tensors():
    """MLP is on the path (every Linear runs on the MFMA kernels): like the CRF / PointConv layers it has no CPU
    route.  Its semantics against the oracle are checked on the GPU (tests/test_gpu_model.py)."""
    from crfconv_amd.models import MLP
    from crfconv_amd._lib import CrfConvError
    m = MLP(12, 20, activation=torch.nn.LeakyReLU(0.1))
    with pytest.raises(CrfConvError, match='no CPU path'):
        m(torch.zeros(3, 50, 12))


WORKER = r'''
import os, sys, torch
sys.path.insert(0, %r)
from crfconv_amd import distributed as D
rank, world, _ = D.init_from_env('gloo')
torch.manual_seed(0)
net = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.LeakyReLU(0.1), torch.nn.Linear(16, 5))
D.broadcast_parameters(net)
bucket = D.FlatGradAllReduce(net)
g = torch.Generator().manual_seed(7)
x = torch.randn(8, 6, generator=g); y = torch.randint(0, 5, (8,), generator=g)
shard = slice(rank * 4, rank * 4 + 4)
bucket.zero()
torch.nn.functional.cross_entropy(net(x[shard]), y[shard]).backward()
bucket.allreduce_mean()
torch.save(torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone(), os.environ['OUT'] + '.%%d' %% rank)
# the failure flag travels with the gradients: rank 1 alone publishes 1, both ranks must see a non-zero slot afterwards
assert float(bucket.guard) == 0.0 and bucket.wire.numel() == bucket.flat.numel() + 1
bucket.publish_guard = lambda: bucket.guard.fill_(float(rank))
bucket.allreduce_sum()
assert float(bucket.guard) == 1.0, float(bucket.guard)
if rank == 0:
    ref = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.LeakyReLU(0.1), torch.nn.Linear(16, 5))
    ref.load_state_dict(net.state_dict())
    torch.nn.functional.cross_entropy(ref(x), y).backward()
    torch.save(torch.cat([p.grad.reshape(-1) for p in ref.parameters()]), os.environ['OUT'] + '.ref')
torch.distributed.barrier()
torch.distributed.destroy_process_group()
'''


def test_sharded_grad_allreduce_equals_big_batch(tmp_path):
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % ROOT)
    env = dict(os.environ, OUT=str(tmp_path / 'g'), MASTER_ADDR='127.0.0.1', MASTER_PORT='29533', WORLD_SIZE='2',
               OMP_NUM_THREADS='1')
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)))
             for r in range(2)]
    for p in procs:
        assert p.wait(timeout=120) == 0
    g0, g1, ref = (torch.load(str(tmp_path / ('g.' + s))) for s in ('0', '1', 'ref'))
    assert torch.equal(g0, g1)                                   # replicas hold identical averaged grads
    assert float((g0 - ref).abs().max()) < 1e-6                  # == gradient of the un-sharded batch


def test_bn_counters_advance_as_one_vector():
    """ops.advance_counters: num_batches_tracked of all BatchNorms advance by one per training forward, survive
    state_dict round trips and module._apply (which breaks the shared storage and must be re-detected)."""
    import torch
    from crfconv_amd import ops
    net = torch.nn.Sequential(torch.nn.BatchNorm1d(4), torch.nn.Linear(4, 4), torch.nn.BatchNorm1d(4))
    net[2].num_batches_tracked += 5
    for expect in (1, 2):
        with ops.advance_counters(net):
            ops.tick(net[0])                                   # inside the context the per-layer tick is a no-op
        assert int(net[0].num_batches_tracked) == expect and int(net[2].num_batches_tracked) == 5 + expect
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    assert sd['0.num_batches_tracked'].shape == () and int(sd['2.num_batches_tracked']) == 7
    net = net.double()                                         # _apply re-creates the buffers one by one
    with ops.advance_counters(net):
        pass
    assert int(net[0].num_batches_tracked) == 3 and int(net[2].num_batches_tracked) == 8
    net.load_state_dict(sd)
    with ops.advance_counters(net):
        pass
    assert int(net[0].num_batches_tracked) == 3 and int(net[2].num_batches_tracked) == 8
    ops.tick(net[0])
    assert int(net[0].num_batches_tracked) == 4


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_module', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                           # (__name__ != '__main__': no self-launch, no benchmark)
    return mod


def test_step_byte_model_reproduces_the_survey_figures():
    """bench.step_byte_model (the algorithmic bytes `roofline_step` is quoted on): the mean-field group must be SURVEY 8(d)'s
    81.9 MB forward for config 2, and its level-0 share the 46.5 MB of `roofline`."""
    bench = _load_bench()
    total, groups = bench.step_byte_model(4, 40960, 16, 3, 13)
    assert abs(groups['mean_field']['fwd'] - 81.9e6) < 0.1e6
    m, H, K, T = 4 * 40960, 8, 16, 3
    assert m * (4 * (K - 1) + 4 * H * (2 * T + 1)) == 46530560
    assert groups['mean_field']['bwd'] == 2 * groups['mean_field']['fwd'] + sum(4 * 40960 // 4 ** l * (4 * K + 4) for l in range(4))
    assert 3.3e9 < total < 3.7e9 and set(groups) == {'encoder_linear', 'pointconv', 'pool_gather', 'decoder_linear', 'mean_field', 'classifier_loss'}
    # scaling sanity: twice the points, twice the bytes
    assert abs(bench.step_byte_model(4, 81920, 16, 3, 13)[0] / total - 2.0) < 1e-9


def test_bench_dump_outputs_keeps_a_fixed_sample_within_its_budget(tmp_path, monkeypatch):
    """bench.dump_outputs (--dump-outputs): arrays under the budget are written whole in float32; over it, each array keeps its share as
    a seeded sample of its flattened elements in ascending order -- the same sample in every call."""
    bench = _load_bench()
    g = torch.Generator().manual_seed(3)
    arrays = {'a': torch.randn(300, 7, generator=g), 'b': torch.randn(100, generator=g, dtype=torch.float64), 'c': torch.tensor(2.5)}
    bench.dump_outputs(str(tmp_path / 'whole'), arrays)
    for k, v in arrays.items():
        a = np.load(str(tmp_path / 'whole' / (k + '.npy')))
        assert a.dtype == np.float32 and a.shape == tuple(v.shape) and np.array_equal(a, v.float().numpy())
    monkeypatch.setattr(bench, 'DUMP_BYTES', 4 * 1000)                # 2201 elements in all -> 1000 kept
    for run in ('s1', 's2'):
        bench.dump_outputs(str(tmp_path / run), arrays)
    files = {k: np.load(str(tmp_path / 's1' / (k + '.npy'))) for k in arrays}
    assert sum(a.nbytes for a in files.values()) <= 4 * 1000
    assert files['a'].shape == (954,) and files['b'].shape == (45,) and files['c'].shape == ()
    assert np.isin(files['a'], arrays['a'].numpy().reshape(-1)).all()
    for k in arrays:
        assert np.array_equal(files[k], np.load(str(tmp_path / 's2' / (k + '.npy'))))


def test_bench_starts_its_own_ranks_without_a_launcher_environment(monkeypatch):
    """`python bench.py --gpus N` with no WORLD_SIZE in the environment: N child processes with the torchrun variables on 127.0.0.1,
    the parent's exit status = the first failing rank's; under a launcher (WORLD_SIZE set) or at N = 1 without --spawn: nothing."""
    bench = _load_bench()
    started = []

    class FakeProc:
        def __init__(self, cmd, env):
            self.cmd, self.env, self.returncode = cmd, env, None
            started.append(self)

        def poll(self):
            self.returncode = 3 if self.env['RANK'] == '1' else 0
            return self.returncode

        def kill(self):
            pass
    import subprocess as sp
    monkeypatch.setattr(sp, 'Popen', FakeProc)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4', '--steps', '2'])
    with pytest.raises(SystemExit) as ex:
        bench._self_launch()
    assert ex.value.code == 3 and len(started) == 4
    assert [p.env['RANK'] for p in started] == ['0', '1', '2', '3'] and [p.env['LOCAL_RANK'] for p in started] == ['0', '1', '2', '3']
    assert all(p.env['WORLD_SIZE'] == '4' and p.env['MASTER_ADDR'] == '127.0.0.1' and p.env['MASTER_PORT'].isdigit() for p in started)
    assert all(p.cmd[0] == sys.executable and p.cmd[1].endswith('bench.py') and p.cmd[2:] == ['--gpus', '4', '--steps', '2'] for p in started)
    del started[:]
    monkeypatch.setenv('WORLD_SIZE', '4')                   # under torchrun: this process IS a rank
    assert bench._self_launch() is None and not started
    monkeypatch.delenv('WORLD_SIZE')
    monkeypatch.setattr(sys, 'argv', ['bench.py'])           # the default N = 1 run stays in-process
    assert bench._self_launch() is None and not started
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--spawn'])
    with pytest.raises(SystemExit):
        bench._self_launch()
    assert len(started) == 1 and started[0].env['WORLD_SIZE'] == '1'


def test_eight_rank_rehearsal_of_the_bench_launch_on_the_cpu(tmp_path):
    """`python bench.py --gpus 8 --rehearse` as the driver would type the 8-GPU command -- no launcher environment,
    bench.py starts the eight ranks itself -- with every rank on the CPU over gloo (eight processes may not share one GPU on this
    pool, and an 8-GPU node is not ours to launch on): port and environment propagation, all ranks joining, the broadcast making the
    replicas equal, the flat all-reduce with its failure-flag slot, the MAX-over-ranks timing and exactly ONE JSON line from rank 0."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'CRFCONV_DIST_BACKEND')}
    env['OMP_NUM_THREADS'] = '1'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '8', '--rehearse', '--steps', '3', '--warmup', '1', '--points', '4096']
    with open(str(tmp_path / 'out'), 'w') as fo, open(str(tmp_path / 'err'), 'w') as fe:
        rc = subprocess.run(cmd, env=env, stdout=fo, stderr=fe, cwd=ROOT, timeout=300).returncode
    assert rc == 0, open(str(tmp_path / 'err')).read()[-3000:]
    lines = [l for l in open(str(tmp_path / 'out')).read().splitlines() if l.startswith('{')]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec['rehearsal'] is True and rec['world'] == 8 and rec['dist_backend'] == 'gloo' and rec['n_gpus'] == 0
    assert rec['replica_spread'] == 0.0 and rec['guard_slot'] == 0.0 and rec['ms_per_step'] > 0
    # a rank that fails must surface as the parent's exit status (and the others must not be left behind)
    bad = subprocess.run(cmd + ['--points', '-5'], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=ROOT, timeout=300)
    assert bad.returncode != 0


def test_tolerances_are_tied_to_the_recorded_errors(monkeypatch):
    """tests/gpu_util.assert_close: with an entry in the baseline (key = test :: what, no occurrence counter) the enforced bound is
    min(stated, max(10 x recorded, noise floor)); the floor is 16 eps where the recorded run was bit-exact; a missing key warns (and
    fails under CRFCONV_TOL_STRICT)."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import gpu_util
    monkeypatch.delenv('CRFCONV_TOL_RECORD', raising=False)
    monkeypatch.delenv('CRFCONV_TOL_STRICT', raising=False)
    gpu_util.set_current_test('tests/x.py::t')
    monkeypatch.setattr(gpu_util, '_baseline', {'tests/x.py::t::a': 1e-6, 'tests/x.py::t::z': 0.0, 'tests/x.py::t::b': 1e-3})
    monkeypatch.setattr(gpu_util, '_warned', set())
    ref = torch.ones(8)
    gpu_util.assert_close(ref + 5e-6, ref, 1e-4, 'a')        # 5e-6 <= 10 x 1e-6
    gpu_util.assert_close(ref + 5e-6, ref, 1e-4, 'a')        # a second call of the same site has the same key, the same bound
    with pytest.raises(AssertionError, match='recorded on MI355X'):
        gpu_util.assert_close(ref + 5e-5, ref, 1e-4, 'a')
    gpu_util.assert_close(ref + 1e-6, ref, 1e-4, 'z')        # recorded 0: floor 16 eps = 1.9e-6, not 1e-7
    with pytest.raises(AssertionError, match='recorded on MI355X'):
        gpu_util.assert_close(ref + 5e-6, ref, 1e-4, 'z')
    gpu_util.assert_close(ref + 5e-5, ref, 1e-4, 'b')        # recorded error above the stated bound: the stated bound rules
    with pytest.raises(AssertionError):
        gpu_util.assert_close(ref + 5e-4, ref, 1e-4, 'b')
    with pytest.warns(UserWarning, match='no recorded error'):
        gpu_util.assert_close(ref + 5e-5, ref, 1e-4, 'unrecorded site')
    monkeypatch.setenv('CRFCONV_TOL_STRICT', '1')
    with pytest.raises(AssertionError, match='CRFCONV_TOL_STRICT'):
        gpu_util.assert_close(ref + 5e-5, ref, 1e-4, 'another unrecorded site')
    baseline = __import__('json').load(open(gpu_util._BASELINE_PATH))
    assert len(baseline) > 2000 and all(v >= 0 for v in baseline.values()) and not any(k.rsplit('#', 1)[-1].isdigit() and '#' in k.rsplit('::', 1)[-1][-4:] for k in baseline)


def test_dropout_mask_host_twin_is_a_keyed_bernoulli_stream():
    """ops.dropout_keep_mask -- the host twin of csrc/common.hpp::dropout_keep (two 32-bit keys per (seed, counter) from one
    splitmix64 round, a two-multiply 32-bit finalizer per element): deterministic, keep rate 1 - p, another mask for another
    counter or seed, no correlation between neighbouring elements or rows, element numbering beyond 2^32 defined."""
    import numpy as np
    from crfconv_amd import ops
    n = 1 << 18
    m = ops.dropout_keep_mask(1234, 7, n, 0.5)
    assert m.dtype == np.bool_ and m.shape == (n,)
    assert np.array_equal(m, ops.dropout_keep_mask(1234, 7, n, 0.5))
    assert abs(m.mean() - 0.5) < 5e-3
    assert abs(ops.dropout_keep_mask(1234, 7, n, 0.3).mean() - 0.7) < 5e-3
    assert ops.dropout_keep_mask(1234, 7, n, 0.0).all()
    for other in (ops.dropout_keep_mask(1234, 8, n, 0.5), ops.dropout_keep_mask(1235, 7, n, 0.5)):
        assert abs((m != other).mean() - 0.5) < 5e-3                # independent fair coins differ half of the time
    for lag in (1, 2, 16, 128):
        c = np.corrcoef(m[:-lag].astype(np.float64), m[lag:].astype(np.float64))[0, 1]
        assert abs(c) < 1e-2, (lag, c)
    # a mask is a function of (seed, counter, element) only: a longer call starts with the shorter one
    assert np.array_equal(ops.dropout_keep_mask(99, 1, 1000, 0.5), ops.dropout_keep_mask(99, 1, 4000, 0.5)[:1000])


def test_graphed_model_state_dict_is_symmetric_as_a_submodule():
    """GraphedModel is transparent for checkpoints -- keys are the wrapped model's -- also when it is a submodule of another module:
    the parent's state_dict() and load_state_dict(strict=True) must agree on the keys (overriding the two methods covered the
    top-level call only)."""
    import torch
    from crfconv_amd.train import GraphedModel

    class Inner(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin, self.bn = torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2)

    class Outer(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.net, self.head = GraphedModel(Inner()), torch.nn.Linear(2, 2)

    inner = Inner()
    g = GraphedModel(inner)
    assert list(g.state_dict().keys()) == list(inner.state_dict().keys())
    g.load_state_dict(inner.state_dict(), strict=True)
    a, b = Outer(), Outer()
    sd = a.state_dict()
    assert 'net.lin.weight' in sd and not any('.model.' in k for k in sd)
    b.load_state_dict(sd, strict=True)
    assert torch.equal(b.net.model.lin.weight, a.net.model.lin.weight) and torch.equal(b.net.model.bn.running_var, a.net.model.bn.running_var)


def test_graphed_model_signature_tells_devices_apart():
    """GraphedModel._signature keys a batch by shape, dtype AND device: a batch of the captured shapes on another device must not be
    load_()-ed into the captured one."""
    import torch
    from crfconv_amd.data import Data
    from crfconv_amd.train import GraphedModel

    def batch(dev, fill=0.0):
        return Data(x=torch.full((2, 5, 6), fill, device=dev), y=torch.zeros(2, 5, dtype=torch.long, device=dev),
                    multiscale=[Data(pos=torch.zeros(2, 5, 3, device=dev))])
    sig = GraphedModel._signature
    assert sig(batch('cpu')) == sig(batch('cpu', 1.0))
    assert sig(batch('cpu')) != sig(batch('meta'))
    assert sig(batch('cpu')) != sig(Data(x=torch.zeros(2, 5, 6), y=torch.zeros(2, 5, dtype=torch.int32),
                                         multiscale=[Data(pos=torch.zeros(2, 5, 3))]))


def test_graphed_model_per_call_checks_see_hooks_and_moved_tensors_after_capture():
    """The per-call checks of GraphedModel.forward over its capture-time snapshot (no GPU needed: the snapshot is all they read):
    hooks registered after the capture -- on any submodule, of every kind, and torch's global module hooks -- and parameters / buffers
    / submodules that are other objects or live at other addresses (p.data = ..., load_state_dict(assign=True), optim.FlatSGD's
    re-homing) are noticed; an in-place load_state_dict is not a move."""
    import torch
    from crfconv_amd.train import GraphedModel

    class Inner(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin, self.bn = torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4)
            self.head = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.ReLU())

    inner = Inner()
    g = GraphedModel(inner, guard_pending=True)

    def snapshot():
        g._snapshot()
        g.fwd_graph = object()                                # (as after a capture: the checks read the snapshot)
        assert not g.hooked() and not g._moved()
    snapshot()
    M = torch.nn.modules.module
    for register in (lambda f: inner.head[0].register_forward_hook(lambda m, i, o: None),
                     lambda f: inner.bn.register_forward_pre_hook(lambda m, i: None),
                     lambda f: inner.lin.register_full_backward_hook(lambda m, gi, go: None),
                     lambda f: inner.register_full_backward_pre_hook(lambda m, go: None),
                     lambda f: M.register_module_forward_hook(lambda m, i, o: None),
                     lambda f: M.register_module_forward_pre_hook(lambda m, i: None),
                     lambda f: M.register_module_full_backward_hook(lambda m, gi, go: None)):
        h = register(None)
        assert g.hooked()
        h.remove()
        assert not g.hooked()
    sd = {k: v.clone() + 1 for k, v in inner.state_dict().items()}
    inner.load_state_dict(sd)                                 # values copied in place: the graphs stay valid
    assert not g._moved()
    inner.head[0].weight.data = inner.head[0].weight.data.clone()
    assert g._moved()
    snapshot()
    inner.bn.running_mean.data = inner.bn.running_mean.clone()
    assert g._moved()
    snapshot()
    inner.load_state_dict({k: v.clone() for k, v in inner.state_dict().items()}, assign=True)
    assert g._moved()
    snapshot()
    inner.load_state_dict(inner.state_dict(), assign=True)    # other Parameter objects over the same storage: still a move
    assert g._moved()
    snapshot()
    inner.head[1] = torch.nn.ReLU()
    assert g._moved()
    snapshot()
    del inner.head[1]
    assert g._moved()
