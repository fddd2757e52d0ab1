"""The sliding block split as far as it goes without a GPU: the NumPy restatement against a loop over all cells and all points, the
new public header's prototypes and record layout, and the conditions on the inputs of tests/test_gpu_sliding_blocks.py -- both drop rules
fire, points lie in as many blocks as the parameters allow, rows sit exactly on a bound, the ragged batch ends one row past a sort
chunk -- so that test cannot hide behind its fixtures."""
import ctypes
import os

import numpy as np
import pytest

from abi_counts import N_FUNCTIONS, N_RECORDS
import sliding_blocks_restatement as R
from crfconv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def scenes():
    return {name: make() for name, make in R.SCENES.items()}


@pytest.mark.parametrize('scene,params', [('carved', 'scannet'), ('carved_small', 's3dis'), ('strip', 'scannet'), ('strip', 'loose'),
                                          ('lattice', 'dyadic'), ('tiny', 'scannet'), ('tiny', 'small_ceil'), ('yard', 'npm3d'),
                                          ('planar', 'small_ceil')])
def test_restatement_is_the_definition(scenes, scene, params):
    p = scenes[scene]
    split = R.np_sliding_blocks(p, **R.PARAM_SETS[params])
    kept = R.brute_sliding_blocks(p, **R.PARAM_SETS[params])
    assert split['n_blocks'] == len(kept) and split['n_rows'] == sum(len(k[2]) for k in kept)
    assert split['cell'].tolist() == [[i, j] for i, j, _, _ in kept]
    assert split['ptr'].tolist() == np.concatenate([[0], np.cumsum([len(k[2]) for k in kept])]).astype(np.int64).tolist()
    assert split['indices'].tolist() == [q for k in kept for q in k[2]]
    assert split['mask'].tolist() == [f for k in kept for f in k[3]]
    assert split['rows'].tolist() == split['indices'].tolist() and split['scene'].tolist() == [0] * len(kept)
    assert split['batch'].tolist() == [b for b, k in enumerate(kept) for _ in k[2]]
    assert split['mask'].dtype == np.int8 and split['cell'].dtype == np.int32 and split['ptr'].dtype == np.int64


def test_restatement_of_a_batch_is_its_scenes_shifted(scenes):
    parts = [scenes['strip'], np.zeros((0, 3), np.float32), scenes['tiny'], scenes['carved_small']]
    ptr = R.ptr_of(parts)
    whole = R.np_sliding_blocks(np.concatenate(parts), ptr, **R.S3DIS)
    b0 = r0 = 0
    for s, p in enumerate(parts):
        one = R.np_sliding_blocks(p, **R.S3DIS)
        sel = slice(r0, r0 + one['n_rows'])
        assert (whole['scene'][b0:b0 + one['n_blocks']] == s).all()
        assert np.array_equal(whole['rows'][sel], one['rows'] + ptr[s]) and np.array_equal(whole['indices'][sel], one['indices'])
        assert np.array_equal(whole['batch'][sel], one['batch'] + b0) and np.array_equal(whole['mask'][sel], one['mask'])
        assert np.array_equal(whole['ptr'][b0:b0 + one['n_blocks'] + 1], one['ptr'] + r0)
        assert np.array_equal(whole['pos_min'][s], one['pos_min'][0]) and np.array_equal(whole['limit'][s], one['limit'][0])
        b0, r0 = b0 + one['n_blocks'], r0 + one['n_rows']
    assert (b0, r0) == (whole['n_blocks'], whole['n_rows'])


def test_count_forms():
    f32 = np.float32
    assert R.axis_blocks(f32(4.3), 1.5, 1.0, 'ratio') == 4 and R.axis_blocks(f32(4.3), 1.5, 1.0, 'ceil_first') == 4
    assert R.axis_blocks(f32(13.0), 5.0, 3.0, 'ratio') == 4 and R.axis_blocks(f32(13.0), 5.0, 3.0, 'ceil_first') == 3    # the parenthesis
    # a scene smaller than block_size - stride: no block under 'ratio'; int() truncates toward zero, so 'ceil_first' may keep one
    assert R.axis_blocks(f32(0.3), 1.5, 1.0, 'ratio') == 0 and R.axis_blocks(f32(0.3), 1.0, 0.5, 'ratio') == 0
    assert R.axis_blocks(f32(0.3), 1.0, 0.5, 'ceil_first') == 1 and R.axis_blocks(f32(0.3), 5.0, 3.0, 'ceil_first') == 0
    assert R.axis_blocks(f32(0.3), 50.0, 1.0, 'ratio') == 0 and R.axis_blocks(f32(0.3), 50.0, 1.0, 'ceil_first') == 0   # below 0 is 0


def test_bounds_are_rounded_once_from_float64():
    lo, hi, clo, chi = R.block_bounds(3, 1.5, 0.1, 0.2)
    assert all(v.dtype == np.float32 for v in (lo, hi, clo, chi))
    beg = 3 * 0.1                                           # 0.30000000000000004: not the float32-rounded product
    assert lo == np.float32(beg - 0.2) and hi == np.float32(beg + 1.5 + 0.2) and clo == np.float32(beg) and chi == np.float32(beg + 1.5)


def test_the_public_block_header_declares_the_entries():
    with open(os.path.join(ROOT, 'include', 'crfconv_amd.h')) as f:
        functions, records = _lib.parse_header(f.read())
    assert len(functions) == N_FUNCTIONS and len(records) == N_RECORDS          # (the first header's counts are pinned: its tables stay its own)
    with open(os.path.join(ROOT, 'include', 'crfconv_blocks.h')) as f:
        functions, records = _lib.parse_header(f.read())
    assert functions == _lib.BLOCKS_SIGNATURES and len(functions) == 5 and list(records) == ['crf_sliding_blocks_spec']
    assert not set(functions) & (set(_lib.SIGNATURES) | set(_lib.INTERNAL_SIGNATURES))
    v, i, l, z, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_double
    assert functions['crfconv_sliding_blocks_workspace'] == (z, [l, l, l])
    assert functions['crfconv_sliding_blocks_count'] == (i, [v, l, v, l, v, l, v, v, v, v, z, v])
    assert functions['crfconv_sliding_blocks_emit_workspace'] == (z, [l, l])
    assert functions['crfconv_sliding_blocks_emit'] == (i, [v, l, v, l, v, l, v, l, l, v, z, v, z, v, v, v, v, v, v, v, v])
    assert functions['crfconv_sliding_blocks_features'] == (i, [v, l, v, v, l, v, i, v, v, v, v, l, l, i, v, v, v, v])
    assert records['crf_sliding_blocks_spec'] == [('block_size', d), ('stride', d), ('padding', d), ('proportion', d), ('min_points', l),
                                                  ('count_form', ctypes.c_int32)]
    spec = _lib.BLOCKS_RECORDS['crf_sliding_blocks_spec']
    assert spec is _lib.SlidingBlocksSpec and ctypes.sizeof(spec) == 48 and spec.min_points.offset == 32 and spec.count_form.offset == 40
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in functions)


def test_the_module_has_the_reference_parameter_sets():
    from crfconv_amd import blocks
    for name, want in R.REFERENCE_SETS.items():
        assert getattr(blocks, name.upper()) == want
    assert blocks.memberships_bound(1.5, 1.0, 0.2) == 9 and blocks.memberships_bound(1.0, 0.5, 0.1) == 16
    assert blocks.memberships_bound(5.0, 3.0, 0.5) == 9 and blocks.memberships_bound(1.0, 0.125, 0.0) == 81


def test_spec_record_layout_matches_the_compiler(tmp_path):
    import shutil
    import subprocess
    cc = next((c for c in ('cc', 'gcc', 'clang') if shutil.which(c)), None)
    assert cc is not None, 'no C compiler on PATH'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "crfconv_blocks.h"', 'int main(void) {']
    for name, cls in _lib.BLOCKS_RECORDS.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f, _ in cls._fields_]
    lines += ['    size_t (*query)(int64_t, int64_t, int64_t) = crfconv_sliding_blocks_workspace; (void)query; return 0;', '}', '']   # (a C caller sees the prototypes)
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.check_call([cc, '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o', str(exe) + '.o'])
    lines[-3] = '    return 0;'
    src.write_text('\n'.join(lines))
    subprocess.check_call([cc, '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    compiled = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    derived = {}
    for name, cls in _lib.BLOCKS_RECORDS.items():
        derived[name] = str(ctypes.sizeof(cls))
        derived.update(('%s.%s' % (name, f), str(getattr(cls, f).offset)) for f, _ in cls._fields_)
    assert derived == compiled and len(derived) == 7


# ------------------------------------------------------------------------------------------- the conditions on the GPU test's inputs
def test_carved_scene_drops_a_block_and_fills_the_multiplicity(scenes):
    p = scenes['carved']
    assert 4500 <= len(p) <= 5500
    split = R.np_sliding_blocks(p, **R.SCANNET)
    assert split['cells'] == 16 and split['dropped_min_points'] >= 1 and split['n_blocks'] >= 12
    assert (R.multiplicity(split, len(p)) == 4).sum() >= 1 and R.max_multiplicity(**R.SCANNET) == 4
    small = scenes['carved_small']
    split = R.np_sliding_blocks(small, **R.S3DIS)
    assert (R.multiplicity(split, len(small)) == 9).sum() >= 1 and R.max_multiplicity(**R.S3DIS) == 9


def test_strip_scene_fires_both_drop_rules(scenes):
    split = R.np_sliding_blocks(scenes['strip'], **R.SCANNET)
    assert split['dropped_min_points'] >= 1 and split['dropped_proportion'] >= 1 and split['n_blocks'] >= 1


def test_lattice_scene_sits_on_the_bounds(scenes):
    p = scenes['lattice']
    assert len(p) < 10000 and np.array_equal(p * 8, np.round(p * 8))
    split = R.np_sliding_blocks(p, **R.DYADIC)
    assert split['on_bound'] >= 100
    # a `>` written for `>=` would lose those rows: the strict test keeps fewer
    a = R.align(p)[0]
    strict = 0
    for b in range(split['n_blocks']):
        i, j = split['cell'][b]
        xl, xh, _, _ = R.block_bounds(i, 1.5, 1.0, 0.25)
        yl, yh, _, _ = R.block_bounds(j, 1.5, 1.0, 0.25)
        strict += int(((a[:, 0] > xl) & (a[:, 0] < xh) & (a[:, 1] > yl) & (a[:, 1] < yh)).sum())
    assert strict == split['n_rows'] - split['on_bound']


def test_tiny_scene_has_no_block_or_one(scenes):
    p = scenes['tiny']
    for name in R.REFERENCE_SETS:
        split = R.np_sliding_blocks(p, **R.PARAM_SETS[name])
        assert split['cells'] == 0 and split['n_blocks'] == 0 and split['n_rows'] == 0 and split['ptr'].tolist() == [0]
    split = R.np_sliding_blocks(p, **R.SMALL_CEIL)
    assert split['cells'] == 1 and split['n_blocks'] == 1 and split['n_rows'] == len(p)


def test_yard_scene_tells_the_count_forms_apart(scenes):
    p = scenes['yard']
    assert R.np_sliding_blocks(p, **R.NPM3D)['cells'] == 9
    assert R.np_sliding_blocks(p, **dict(R.NPM3D, count_form='ratio'))['cells'] == 12
    assert R.np_sliding_blocks(p, **R.NPM3D)['n_blocks'] >= 4


def test_planar_scene_has_no_height(scenes):
    p = scenes['planar']
    split = R.np_sliding_blocks(p, **R.S3DIS)
    assert split['limit'][0, 2] == 0 and split['n_blocks'] >= 4
    x = R.np_features(p, None, split, 'room')[1]
    assert np.isnan(x[:, 2]).all() and np.isfinite(x[:, :2]).all()


def test_ragged_batch_has_every_size_and_ends_one_past_a_chunk():
    parts = R.ragged_scenes()
    sizes = [len(p) for p in parts]
    assert sizes[:5] == [0, 1, 63, 65, 1025] and 4100 <= sizes[5] <= 4100 + R.SORT_CHUNK and max(sizes) < 10000
    assert sizes[6] == len(R.tiny_scene()) and sizes[7] == len(R.strip_scene())
    pos, ptr = np.concatenate(parts), R.ptr_of(parts)
    split = R.np_sliding_blocks(pos, ptr, **R.SCANNET)
    assert split['n_rows'] > 3 * R.SORT_CHUNK and split['n_rows'] % R.SORT_CHUNK == 1
    assert split['dropped_min_points'] >= 1 and split['dropped_proportion'] >= 1
    # rows are not sorted along x inside the scenes (the emission order is the point order, not a spatial one)
    big = pos[ptr[5]:ptr[6], 0]
    assert (np.diff(big) < 0).sum() > len(big) // 4
    loose = R.np_sliding_blocks(pos, ptr, **R.LOOSE)
    # (the empty scene, the one-point scene -- its extent is 0 -- and the tiny scene have no block under 'ratio')
    assert set(loose['scene'].tolist()) == {2, 3, 4, 5, 7} and loose['n_blocks'] > 64
