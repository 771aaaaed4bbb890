"""The tensor checks of the host layer, written once, beside the scalar ones of _check.py: "a tensor of this dtype, usable in
place", "a batch of images", "range images (...,H,W,3) the kernels' int indices can address", "[q | t] rows of this shape", "all on
one device".  What the front ends of _scan_ops.py -- and the products built on them -- can refuse without a GPU or the library.
A wrong type is a TypeError, a wrong value the `kind` asked for (EloError: the front ends'; ValueError: the products'); a message
is built only where one is raised."""
import torch

from ._lib import EloError


def tensors(given):
    """Each (name, tensor, dtype) of `given` is a tensor of that dtype (TypeError) that the launch can use in place (EloError)."""
    for name, t, dtype in given:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s is a tensor (got %r)" % (name, type(t).__name__))
        if t.dtype != dtype:
            raise TypeError("%s is %s (got %s)" % (name, str(dtype).replace("torch.", ""), t.dtype))
        if not t.is_contiguous():
            raise EloError("%s must be contiguous: the launch uses it in place" % name)


def range_images(name, t, layout, min_h=1, min_w=1, below=()):
    """The tensor `t` holds range images: one size per letter of `layout` and then 3 -- "BKHW": (B,K,H,W,3) --, at least min_h x
    min_w cells each, and every product of sizes `below` names ("KHW", "BHW") below 2^31 -> the sizes, in layout's order."""
    shape = t.shape
    if len(shape) != len(layout) + 1 or shape[-1] != 3:
        raise EloError("%s is (%s,3): range images (got %s)" % (name, ",".join(layout), tuple(shape)))
    if shape[-3] < min_h or shape[-2] < min_w:
        raise EloError("%s has no cells for this: H >= %d, W >= %d (got %d x %d)" % (name, min_h, min_w, shape[-3], shape[-2]))
    for product in below:
        cells = 1
        for size in product:
            cells *= shape[layout.index(size)]
        if cells >= 2 ** 31:
            raise EloError("%s stays below 2^31 (got %s = %s for %s)" % ("*".join(product), ",".join(layout), tuple(shape[:-1]), name))
    return shape[:-1]


def image_batch(name, t, kind=ValueError):
    """`t` is a tensor of four dimensions -- (n,H,W,3) range images, by what the front end it goes to checks next -> n: what a
    product asks before it counts its images."""
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        raise kind("%s is an (n,H,W,3) tensor of range images (got %r)" % (name, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
    return t.shape[0]


def pose_rows(name, t, shape, per, kind=EloError):
    """The tensor `t` is [q | t] rows of exactly `shape`, (...,7): one row per `per` ("image", "slot", ...)."""
    if t.shape != shape:
        raise kind("%s is one [q0 q1 q2 q3 | t0 t1 t2] row per %s: %s (got %s)" % (name, per, shape, tuple(t.shape)))


def one_device(what, first, *others):
    """Every tensor of `others` lives where `first` does; `what` names them all."""
    device = first.device
    for t in others:
        if t.device != device:
            raise EloError("%s live on one device (got %s and %s)" % (what, device, t.device))
