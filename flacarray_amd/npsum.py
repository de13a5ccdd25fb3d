"""numpy's summation order for `np.std(x, axis=-1)`, as a plan and as a vectorised CPU model.

numpy reduces a C-contiguous row in chunks of `np.getbufsize()` elements (relative to the row start).  Each chunk is
summed by `@TYPE@_pairwise_sum` (numpy/_core/src/umath/loops_utils.h.src), and the chunk sums are added one after the
other, starting from 0.  `np.std` then computes, all in the data dtype unless said otherwise:

    mean = dtype(float64(sum(x)) / n)      d = dtype(x - mean)      d2 = dtype(d * d)
    var  = dtype(float64(sum(d2)) / n)     std = sqrt(var)

`pairwise_plan` gives the tree of one chunk, which the device kernel (csrc/std_kernels.hpp) follows for every chunk
that is not a full 8192-element one; `std_model` executes the whole recipe in numpy, the yardstick of the kernel's
bits next to `np.std` itself.
"""
import numpy as np

LEAF = 128  # pairwise_sum sums at most this many elements without splitting
FAST_CHUNK = 8192  # 64 leaves of 128: the kernel's lane-per-leaf path


def pairwise_plan(length):
    """The leaves and combine order of numpy's pairwise sum over `length` elements.

    Returns (leaves, ops): `leaves` an int64 array (k, 2) of (offset, length) in element order; `ops` a uint8 postfix
    program over them, 1 = push the next leaf's sum, 0 = pop two sums and push their sum.  A leaf of fewer than 8
    elements (only a whole chunk that short) is summed in order from -0.0; a leaf of 8 to 128 elements with eight
    strided accumulators, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then its n % 8 remaining elements in order."""
    length = int(length)
    if length <= 0:
        raise ValueError("pairwise_plan needs a positive length")
    leaves, ops = [], []
    stack = [(0, length, False)]
    while stack:  # explicit post-order walk: (offset, n, children already emitted)
        off, n, done = stack.pop()
        if n <= LEAF:
            leaves.append((off, n))
            ops.append(1)
        elif done:
            ops.append(0)
        else:
            n2 = n // 2
            n2 -= n2 % 8
            stack.append((off, n, True))
            stack.append((off + n2, n - n2, False))
            stack.append((off, n2, False))
    return np.array(leaves, dtype=np.int64).reshape(-1, 2), np.array(ops, dtype=np.uint8)


def _leaf_sum(a):
    """pairwise_sum of the last axis of `a` for a leaf (at most 128 elements), vectorised over the leading axes."""
    n = a.shape[-1]
    if n < 8:
        res = np.full(a.shape[:-1], -0.0, dtype=a.dtype)
        for i in range(n):
            res = res + a[..., i]
        return res
    r = a[..., 0:8].copy()
    stop = n - n % 8
    for i in range(8, stop, 8):
        r += a[..., i : i + 8]
    res = ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))
    for i in range(stop, n):
        res = res + a[..., i]
    return res


def pairwise_sum(a):
    """numpy's pairwise sum of the last axis of `a` (one chunk), vectorised over the leading axes."""
    leaves, ops = pairwise_plan(a.shape[-1])
    stack, k = [], 0
    for op in ops:
        if op:
            off, n = leaves[k]
            stack.append(_leaf_sum(a[..., off : off + n]))
            k += 1
        else:
            right = stack.pop()
            stack.append(stack.pop() + right)
    return stack[0]


def chunked_sum(x, bufsize=None):
    """Sum of the last axis the way a numpy reduction of a contiguous row does it: pairwise sums of consecutive chunks
    of `bufsize` elements (np.getbufsize() by default), folded in order starting from 0."""
    b = int(np.getbufsize() if bufsize is None else bufsize)
    n = x.shape[-1]
    full = n // b
    s = np.zeros(x.shape[:-1], dtype=x.dtype)
    if full:
        sums = pairwise_sum(x[..., : full * b].reshape(x.shape[:-1] + (full, b)))
        for c in range(full):
            s = s + sums[..., c]
    if n > full * b:
        s = s + pairwise_sum(x[..., full * b :])
    return s


def std_model(x, bufsize=None):
    """`np.std(x, axis=-1)` of a float32 / float64 array, bit for bit, from the recipe in this module's docstring."""
    x = np.ascontiguousarray(x)
    if x.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("std_model takes float32 or float64 data")
    dt = x.dtype.type
    n = np.float64(x.shape[-1])
    mean = (chunked_sum(x, bufsize).astype(np.float64) / n).astype(dt)
    d = x - mean[..., None]
    var = (chunked_sum(d * d, bufsize).astype(np.float64) / n).astype(dt)
    return np.sqrt(var)
