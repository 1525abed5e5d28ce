"""CPU: the host side of pool training (include/gfv.h gfv_pool_*, gfv.pool.BatchArena): the new entry points are declared,
exported and bound, every bad argument is refused before anything touches a device, and the signature / capacity arithmetic."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cases

NEW = ("gfv_pool_args_bytes", "gfv_pool_table_bytes", "gfv_pool_table_check", "gfv_pool_assemble", "gfv_pool_payback")


def test_pool_entry_points_are_declared_exported_and_bound():
    from gfv import lib
    handle = lib.load()
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    declared = set(re.findall(r"\b(gfv_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in lib.declared_symbols() and hasattr(handle, name), name
        assert getattr(handle, name).argtypes is not None
    assert handle.gfv_abi_version() == 3                                   # additive: the version stays
    assert handle.gfv_pool_args_bytes() == C.sizeof(lib.PoolArgs)
    assert handle.gfv_pool_table_bytes(3, 43) == 3 * (lib.POOL_ROW_HEAD + 2 * 43) * 8
    for k in ("GFV_POOL_MAX_GRAPHS", "GFV_POOL_MAX_ATTRS", "GFV_POOL_ROW_HEAD"):
        assert int(re.search(rf"#define {k} (\d+)", header).group(1)) == getattr(lib, k[4:])


def _table(sizes, n_attrs=3):
    """A hand-made table: attribute 0 = node ids (one word per node, offset by nodes), 1 = a row pointer over the nodes with
    face non-zeros, 2 = a graph-id fill per node.  The pointers are fake (nothing is launched)."""
    from gfv import lib
    row = lib.POOL_ROW_HEAD + 2 * n_attrs
    tab = np.zeros((len(sizes), row), dtype=np.int64)
    for i, (n, e) in enumerate(sizes):
        tab[i, 0:6] = (n, e, 0, 0, 0, (n + 63) // 64)
        tab[i, lib.POOL_ROW_HEAD:lib.POOL_ROW_HEAD + 2] = 0x10000 * (i + 1), 0x20000 * (i + 1)
        tab[i, lib.POOL_ROW_HEAD + n_attrs:] = (n, n + 1, n)
    info = (C.c_int32 * n_attrs)(lib.POOL_ADD | (1 << 4), lib.POOL_ROWPTR | (2 << 4), lib.POOL_FILL)
    return np.ascontiguousarray(tab), info


def _args(tab, info, cap_nodes=300, max_graphs=4):
    from gfv import lib
    a = lib.PoolArgs()
    a.table_host, a.table_dev = tab.ctypes.data, 0x7000000
    a.n_entries, a.n_attrs, a.max_graphs, a.slice_chunk, a.max_chunks = tab.shape[0], len(info), max_graphs, 64, 8
    for j in range(len(info)):
        a.attr_info[j], a.dst[j], a.dst_cap_words[j] = info[j], 0x100000 * (j + 1), cap_nodes + (1 if j == 1 else 0)
    for k in range(6):
        a.small[k] = 0x900000 + 0x1000 * k
    a.B = 2
    a.idx[0], a.idx[1] = 0, 1
    return a


def test_pool_entry_points_refuse_bad_arguments_without_a_gpu():
    """Each case differs from an acceptable call in ONE argument (the acceptable call itself cannot be issued without a device;
    tests/test_pool_train_gpu.py runs it)."""
    from gfv import lib
    handle = lib.load()
    tab, info = _table([(100, 250), (120, 310), (90, 200)])
    assert handle.gfv_pool_table_check(tab.ctypes.data, 3, 3, C.addressof(info)) == 0
    assert handle.gfv_pool_table_check(None, 3, 3, C.addressof(info)) == -1
    assert handle.gfv_pool_table_check(tab.ctypes.data, 0, 3, C.addressof(info)) == -1
    assert handle.gfv_pool_table_check(tab.ctypes.data, 3, lib.POOL_MAX_ATTRS + 1, C.addressof(info)) == -1
    bad = tab.copy()
    bad[1, lib.POOL_ROW_HEAD] = 0                                           # words without a source
    assert handle.gfv_pool_table_check(bad.ctypes.data, 3, 3, C.addressof(info)) == -1
    bad = tab.copy()
    bad[2, lib.POOL_ROW_HEAD + 1] += 2                                      # a source that is not word aligned
    assert handle.gfv_pool_table_check(bad.ctypes.data, 3, 3, C.addressof(info)) == -1
    bad = tab.copy()
    bad[0, 0] = -1
    assert handle.gfv_pool_table_check(bad.ctypes.data, 3, 3, C.addressof(info)) == -1

    asm = lambda a: handle.gfv_pool_assemble(C.byref(a), None)
    assert handle.gfv_pool_assemble(None, None) == -1
    a = _args(tab, info)
    a.table_host = None                                                     # null table
    assert asm(a) == -1
    a = _args(tab, info)
    a.table_dev = None
    assert asm(a) == -1
    for B in (0, -3, 5, lib.POOL_MAX_GRAPHS + 1):                           # B < 1, B above the arena's capacity of 4 graphs
        a = _args(tab, info)
        a.B = B
        assert asm(a) == -1, B
    for i in (-1, 3, 1 << 20):                                              # an index outside the pool
        a = _args(tab, info)
        a.idx[1] = i
        assert asm(a) == -1, i
    a = _args(tab, info, cap_nodes=219)                                     # 100 + 120 nodes do not fit 219 words
    assert asm(a) == -1
    a = _args(tab, info)
    a.max_chunks = 3                                                        # 2 + 2 chunks of 64 nodes
    assert asm(a) == -1
    a = _args(tab, info)
    a.dst[0] = 0x100004                                                     # destinations are 16-byte aligned
    assert asm(a) == -1
    a = _args(tab, info)
    a.small[4] = None
    assert asm(a) == -1

    idx = (C.c_int32 * 2)(0, 1)
    uvp, tdev = 0x5000000, 0x7000000
    tabx, _ = _table([(100, 250), (120, 310)])
    tabx[:, lib.POOL_ROW_HEAD + 3] = 12 * tabx[:, 0]                        # attribute 0 as an [n, 12] node state
    pay = lambda **kw: handle.gfv_pool_payback(*[kw.get(k, d) for k, d in (
        ("host", tabx.ctypes.data), ("dev", tdev), ("n", 2), ("A", 3), ("x", 0), ("idx", C.addressof(idx)), ("B", 2), ("uvp", uvp),
        ("N", 220), ("raw", None), ("stream", None))])
    assert pay(host=None) == -1 and pay(dev=None) == -1 and pay(idx=None) == -1 and pay(uvp=None) == -1
    assert pay(B=0) == -1 and pay(B=lib.POOL_MAX_GRAPHS + 1) == -1
    assert pay(x=3) == -1 and pay(x=-1) == -1 and pay(x=1) == -1           # (attribute 1 is not an [n, 12] state)
    assert pay(N=219) == -1 and pay(N=0) == -1
    outside = (C.c_int32 * 2)(0, 2)
    assert pay(idx=C.addressof(outside)) == -1


def test_signature_and_capacity_arithmetic():
    from gfv.pool import batch_signature, batch_totals, check_fits, default_capacity, entry_signature
    mk = lambda n, e, c, k, s: dict(n=n, e=e, e2=2 * e, c=c, k=k, s=s, nchunk=(n + 63) // 64)
    sizes = [mk(217, 574, 357, 1071, 4948), mk(64, 126, 63, 224, 1108), mk(217, 573, 356, 1068, 4940), mk(217, 574, 357, 1071, 4948)]
    assert entry_signature(sizes[0]) == (217, 574, 357, 1071, 4948, 4)
    assert batch_signature(sizes, [0, 1]) == batch_signature(sizes, [3, 1])          # equal sizes, other entries
    assert batch_signature(sizes, [0, 1]) != batch_signature(sizes, [1, 0])          # the signature is ordered
    assert batch_signature(sizes, [0]) != batch_signature(sizes, [2])                # 574 against 573 faces
    assert batch_totals(sizes, [0, 1, 1]) == dict(n=345, e=826, c=483, k=1519, s=7164, nchunk=6)
    cap = default_capacity(sizes, 2)
    assert cap == dict(n=434, e=1148, c=714, k=2142, s=9896, nchunk=8)
    check_fits(batch_totals(sizes, [0, 3]), 2, cap, 2)                              # exactly the capacity
    check_fits(batch_totals(sizes, [1]), 1, cap, 2)
    with pytest.raises(ValueError):
        check_fits(batch_totals(sizes, [0, 3, 1]), 3, cap, 2)                       # more graphs than the arena holds
    with pytest.raises(ValueError):
        check_fits(batch_totals(sizes, [0, 3]), 2, dict(cap, s=9895), 2)            # one size one short
    with pytest.raises(ValueError):
        check_fits(batch_totals(sizes, []), 0, cap, 2)
    with pytest.raises(ValueError):
        default_capacity(sizes, 0)


def test_meshes_of_the_gpu_tests_have_the_signatures_they_rely_on():
    """tests/test_pool_train_gpu.py: three jittered cavities share one size signature; the two cylinder meshes differ by one face."""
    from gfv import meshgen
    from gfv.pool import DevicePool, batch_signature
    raws = [meshgen.raw_quad_cavity(n=7, jitter=0.1, tri_fraction=0.3, seed=s) for s in (13, 14, 15)]
    raws += [meshgen.raw_tri_channel_cylinder(nx=30, ny=6, seed=s) for s in (21, 22)]
    pool = DevicePool([meshgen.finish_mesh(r, U=1.0) for r in raws], device="cpu")
    sig = [batch_signature(pool.sizes, [i]) for i in range(5)]
    assert sig[0] == sig[1] == sig[2] and sig[0][0][:4] == (64, 126, 63, 224)
    assert (pool.sizes[3]["e"], pool.sizes[4]["e"]) == (574, 573) and sig[3] != sig[4]
    # a variant shares the structure of its parent and owns its boundary condition; an arena over the pool sees it
    v = pool.add_variant(3, U=0.3, mu=2e-3, dt=0.02)
    assert pool.plans[v].es.data_ptr() == pool.plans[3].es.data_ptr() and pool.plans[v].theta.data_ptr() != pool.plans[3].theta.data_ptr()
    arena = pool.arena(2)
    assert arena.signature([v, 0]) == arena.signature([3, 1])
    with pytest.raises(ValueError):
        arena.load([3, 4, 0])
    with pytest.raises(ValueError):
        arena.load([9])
