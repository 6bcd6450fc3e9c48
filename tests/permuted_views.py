"""A 4-D tensor laid out so that a slip in a kernel's row addressing shows: ne[2] > 1 and ne[3] > 1, rows padded (nb[1] is larger than the row) and dimension 2
outermost in memory (nb[2] > nb[3]: a permuted view), so no two strides are equal and none follows from the shape.  The row-wise ops (and GROUP_NORM, group-wise)
compute the same words whatever the layout: the expected result is the CPU oracle's over the same values gathered into a contiguous tensor."""
import numpy as np

FILL = 7.0


def permuted(gpu, x, pad):
    """x: [ne3, ne2, ne1, ne0] on the host.  Returns (view, read): the device tensor [ne0, ne1, ne2, ne3] over a buffer [ne2][ne3][ne1][ne0 + pad] that holds x, FILL
    between the rows; read() gathers what the view holds now into x's shape and checks that nothing was written between the rows"""
    ne3, ne2, ne1, ne0 = x.shape
    host = np.full((ne2, ne3, ne1, ne0 + pad), FILL, x.dtype)
    host[..., :ne0] = x.transpose(1, 0, 2, 3)
    row = (ne0 + pad) * x.dtype.itemsize
    buf = gpu.Tensor.from_numpy(host)
    view = buf.view([ne0, ne1, ne2, ne3], [x.dtype.itemsize, row, ne3 * ne1 * row, ne1 * row])

    def read():
        got = buf.numpy().reshape(host.shape)
        assert np.array_equal(got[..., ne0:], host[..., ne0:]), "a store between the rows"
        return np.ascontiguousarray(got[..., :ne0].transpose(1, 0, 2, 3))
    return view, read
