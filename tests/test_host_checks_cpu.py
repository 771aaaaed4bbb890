"""CPU: the checks the host layer spells once -- _check.py's scalars (no torch), _check_torch.py's tensors -- and where the
scan-level front ends and the pose algebra live after their move (_scan_ops.py, pose7.py)."""
import ast
import math

import numpy as np
import pytest
import torch

from conftest import load_pkg

KINDS = (ValueError, TypeError, load_pkg("_lib").EloError)
MOVED = ("pose_fit", "model_render", "model_begin", "model_advance", "map_insert", "map_extract", "map_merge", "map_fit",
         "scan_descriptor", "descriptor_search", "PoseFitResult", "MapFitResult", "PlaceSearchResult")


@pytest.mark.parametrize("kind", KINDS)
def test_integer(kind):
    integer = load_pkg("_check").integer
    for good in (3, np.int64(3), 7, np.int32(7)):
        got = integer("n", good, kind, 3, 7)
        assert type(got) is int and got == good                                          # both bounds inclusive
    assert integer("n", -5, kind) == -5 and integer("n", 2 ** 70, kind, 0) == 2 ** 70     # an open end
    for bad in (True, False, 1.0, "1", None, np.float64(4.0), 3 - 1, 7 + 1):
        with pytest.raises(kind, match="n is an integer") as e:
            integer("n", bad, kind, 3, 7)
        assert type(e.value) is kind and repr(bad) in str(e.value)


@pytest.mark.parametrize("kind", KINDS)
def test_real(kind):
    real = load_pkg("_check").real
    for good in (1.5, 2, np.float32(0.25), np.float64(1e300), -3.0, 0.0, "2.5"):
        got = real("x", good, kind)
        assert type(got) is float and got == float(good)
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(kind, match="^x must be finite") as e:
            real("x", bad, kind)
        assert type(e.value) is kind
    assert real("x", math.inf, kind, finite=False) == math.inf
    assert real("x", math.inf, kind, finite=False, positive=True) == math.inf
    with pytest.raises(kind):
        real("x", math.nan, kind, finite=False)
    for bad in (math.nan, math.inf, -0.0, 0.0, -1.0):
        with pytest.raises(kind, match="x must be finite and positive") as e:
            real("x", bad, kind, positive=True)
        assert type(e.value) is kind
    assert real("x", 1e-300, kind, positive=True) == 1e-300
    assert real("x", 0.0, kind, non_negative=True) == 0.0 and real("x", -0.0, kind, non_negative=True) == 0.0
    for bad in (-1e-300, math.nan, math.inf):
        with pytest.raises(kind):
            real("x", bad, kind, non_negative=True)
    # a bool is a number to float(): it passes where today's values take it, and is refused where they refuse it
    assert real("x", True, kind) == 1.0
    for takes in ("no_bool", "numbers"):
        for bad in (True, False):
            with pytest.raises(kind, match="x is a number") as e:
                real("x", bad, kind, takes=takes)
            assert type(e.value) is kind
    assert real("x", np.float32(0.5), kind, takes="no_bool") == 0.5 and real("x", "0.5", kind, takes="no_bool") == 0.5
    # what float() does not take is float()'s own error, as the values have always let it through ...
    for takes in ("any", "no_bool"):
        with pytest.raises(TypeError, match="float"):
            real("x", None, kind, takes=takes)
        with pytest.raises(ValueError, match="float"):
            real("x", "metres", kind, takes=takes)
    # ... but where only numbers are asked for: python ints and floats (numpy.float64 is one), everything else is a `kind`
    assert real("x", 40, kind, takes="numbers") == 40.0 and real("x", np.float64(2.5), kind, takes="numbers") == 2.5
    for bad in (None, "40", np.float32(40.0), [40.0], 1 + 0j):
        with pytest.raises(kind, match="x is a number") as e:
            real("x", bad, kind, takes="numbers")
        assert type(e.value) is kind


def test_where_a_bool_is_refused_today():
    S = load_pkg("sensor")
    assert S.PoseFit(gate=True).gate == 1.0 and S.VoxelMap(voxel=True).voxel == 1.0 and S.Sensor(crop_xy=True).crop_xy == 1.0
    for bad in (lambda: S.MapWindow(True), lambda: S.ScanContext(max_range=True), lambda: S.ScanContext(min_range=False),
                lambda: S.ScanContext(z_min=True), lambda: S.ScanContext(z_step=True)):
        with pytest.raises(ValueError):
            bad()
    assert S.Sensor(crop_xy=math.inf).crop_xy == math.inf and S.VoxelMap(max_range=math.inf).max_range == math.inf
    for bad in (lambda: S.PoseFit(gate=None), lambda: S.VoxelMap(voxel=None), lambda: S.Sensor(crop_xy=[35.0])):   # float()'s own
        with pytest.raises(TypeError):
            bad()


def test_is_a():
    is_a, S = load_pkg("_check").is_a, load_pkg("sensor")
    fit = S.PoseFit()
    assert is_a("fit", fit, S.PoseFit) is fit and is_a("fit", fit, S.PoseFit, or_none=True) is fit
    assert is_a("fit", None, S.PoseFit, or_none=True) is None
    with pytest.raises(TypeError, match=r"fit is a PoseFit \(got 'NoneType'\)"):
        is_a("fit", None, S.PoseFit)
    with pytest.raises(TypeError, match=r"fit is a PoseFit or None \(got 'dict'\)"):
        is_a("fit", {}, S.PoseFit, or_none=True)
    with pytest.raises(ValueError, match=r"context is a ScanContext \(got 'MapFit'\)"):
        is_a("context", S.MapFit(), S.ScanContext, ValueError)
    with pytest.raises(TypeError):                                                        # (another value class with the same fields)
        is_a("fit", S.PoseFit(), S.MapFit)


def test_the_scalar_checks_and_the_values_need_neither_torch_nor_the_library():
    """(The package's __init__ imports torch, so the two modules are read as files: what they import is all there is to ask.)"""
    for module, allowed in (("_check", {"math"}), ("sensor", {"math", "_check"})):
        with open(load_pkg(module).__file__) as f:
            tree = ast.parse(f.read())
        names = set()
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                names.update(alias.name for alias in node.names)
            elif isinstance(node, ast.ImportFrom):
                names.add(node.module or ".")
        assert names <= allowed, (module, names)


def test_tensors():
    T, L = load_pkg("_check_torch"), load_pkg("_lib")
    x = torch.zeros((2, 4, 8, 3))
    T.tensors((("x", x, torch.float32), ("n", torch.zeros(3, dtype=torch.int64), torch.int64)))
    for bad in (x.numpy(), None, [0.0]):
        with pytest.raises(TypeError, match="x is a tensor"):
            T.tensors((("x", bad, torch.float32),))
    with pytest.raises(TypeError, match="x is float32 .got torch.float64"):
        T.tensors((("x", x.double(), torch.float32),))
    with pytest.raises(L.EloError, match="x must be contiguous"):
        T.tensors((("x", x.transpose(1, 2), torch.float32),))
    with pytest.raises(TypeError, match="y is int32"):                                    # every entry is looked at, in order
        T.tensors((("x", x, torch.float32), ("y", x, torch.int32)))


def test_range_images():
    T, L = load_pkg("_check_torch"), load_pkg("_lib")
    x = torch.zeros((2, 4, 8, 3))
    assert tuple(T.range_images("x", x, "BHW")) == (2, 4, 8)
    assert tuple(T.range_images("x", x.reshape(1, 2, 4, 8, 3), "BKHW", min_h=4, min_w=8, below=("KHW", "BHW"))) == (1, 2, 4, 8)
    for bad in (torch.zeros((2, 4, 8, 4)), torch.zeros((2, 4, 8, 2)), torch.zeros((4, 8, 3)), torch.zeros((1, 2, 4, 8, 3))):
        with pytest.raises(L.EloError, match=r"x is \(B,H,W,3\): range images \(got \(.*\)\)"):
            T.range_images("x", bad, "BHW")
    with pytest.raises(L.EloError, match=r"x has no cells for this: H >= 5, W >= 1 \(got 4 x 8\)"):
        T.range_images("x", x, "BHW", min_h=5)
    with pytest.raises(L.EloError, match=r"H >= 1, W >= 9 \(got 4 x 8\)"):
        T.range_images("x", x, "BHW", min_w=9)
    for empty in (torch.zeros((2, 4, 0, 3)), torch.zeros((2, 0, 8, 3))):
        with pytest.raises(L.EloError, match="x has no cells"):
            T.range_images("x", empty, "BHW")
    assert tuple(T.range_images("x", torch.zeros((0, 4, 8, 3)), "BHW", below=("BHW",))) == (0, 4, 8)     # no image is no error
    # 2^31 cells are one too many for the kernels' int indices; nothing is allocated for the question
    meta = lambda *shape: torch.empty(shape + (3,), device="meta")
    assert tuple(T.range_images("x", meta(1, 1, 2 ** 31 - 1), "BHW", below=("BHW",))) == (1, 1, 2 ** 31 - 1)
    for shape in ((1, 1, 2 ** 31), (2, 2 ** 15, 2 ** 15), (1, 2 ** 16, 2 ** 15 + 1)):
        with pytest.raises(L.EloError, match=r"B\*H\*W stays below 2\^31 \(got B,H,W = \(%d, %d, %d\) for x\)" % shape):
            T.range_images("x", meta(*shape), "BHW", below=("BHW",))
        assert tuple(T.range_images("x", meta(*shape), "BHW")) == shape                   # (asked of nothing, nothing is refused)
    # each named product by itself: B*K*H*W may pass 2^31 where K*H*W and B*H*W do not
    big = meta(2 ** 10, 2 ** 4, 2 ** 10, 2 ** 10)
    assert tuple(T.range_images("src", big, "BKHW", below=("KHW", "BHW"))) == (2 ** 10, 2 ** 4, 2 ** 10, 2 ** 10)
    with pytest.raises(L.EloError, match=r"K\*H\*W stays below 2\^31"):
        T.range_images("src", meta(1, 2 ** 11, 2 ** 10, 2 ** 10), "BKHW", below=("KHW", "BHW"))
    with pytest.raises(L.EloError, match=r"B\*H\*W stays below 2\^31"):
        T.range_images("src", meta(2 ** 11, 1, 2 ** 10, 2 ** 10), "BKHW", below=("KHW", "BHW"))


def test_image_batch():
    T = load_pkg("_check_torch")
    assert T.image_batch("xyz", torch.zeros((2, 4, 8, 3))) == 2 and T.image_batch("xyz", torch.empty((0, 1, 1, 3), device="meta")) == 0
    for bad, got in ((torch.zeros((4, 8, 3)), r"\(4, 8, 3\)"), (torch.zeros((1, 2, 4, 8, 3)), r"\(1, 2, 4, 8, 3\)"), (np.zeros((2, 4, 8, 3)), "'ndarray'"),
                     (None, "'NoneType'")):
        with pytest.raises(ValueError, match=r"xyz is an \(n,H,W,3\) tensor of range images \(got %s\)" % got):
            T.image_batch("xyz", bad)
    with pytest.raises(TypeError):
        T.image_batch("xyz", None, TypeError)


def test_pose_rows_and_one_device():
    T, L = load_pkg("_check_torch"), load_pkg("_lib")
    T.pose_rows("pose", torch.zeros((2, 7)), (2, 7), "image")
    T.pose_rows("pose", torch.zeros((2, 3, 7), dtype=torch.float64), (2, 3, 7), "source")
    for bad in (torch.zeros((3, 7)), torch.zeros((2, 4)), torch.zeros((2, 8)), torch.zeros(7), torch.zeros((1, 2, 7))):
        with pytest.raises(L.EloError, match=r"pose is one \[q0 q1 q2 q3 \| t0 t1 t2\] row per image: \(2, 7\) \(got \(.*\)\)"):
            T.pose_rows("pose", bad, (2, 7), "image")
        with pytest.raises(ValueError, match="row per scan"):
            T.pose_rows("pose", bad, (2, 7), "scan", ValueError)
    a, b, c = torch.zeros(3), torch.zeros((2, 2)), torch.empty(4, device="meta")
    T.one_device("a and b", a, b)
    T.one_device("a", a)
    for others in ((c,), (b, c), (c, b)):
        with pytest.raises(L.EloError, match=r"a, b and c live on one device \(got cpu and meta\)"):
            T.one_device("a, b and c", a, *others)


def test_one_name_one_home():
    ops, scan, pose7 = load_pkg("_ops"), load_pkg("_scan_ops"), load_pkg("pose7")
    assert [name for name in MOVED if hasattr(ops, name)] == [] and [name for name in MOVED if not hasattr(scan, name)] == []
    assert not hasattr(ops, "_check_tensors") and scan.cell_rule is ops.cell_rule
    assert load_pkg("world_map").compose is pose7.compose and load_pkg("local_model").rebase is pose7.rebase
    assert not hasattr(load_pkg("local_model"), "_qmul") and not hasattr(load_pkg("world_map"), "_qmul")
