"""NumPy statement of the index map that the training kernels of the un-rotation use (csrc/elem.hip: rot_dst;
csrc/conv.hip: unrot_act_bwd64_kernel), the model of tests/test_unrot_map_cpu.py.

Stack plane (n = kB + b, c), element (s, v), belongs to element (i, j) of plane (b, kC + c) of the un-rotated tensor f:
the plane is shifted down one row (row P-1 is dropped, row 0 of the shifted plane is zero) and turned clockwise by
a_k = (0, 270, 180, 90)[k] degrees.  The same map is the store address of a forward kernel that writes f directly and
the gather address of the backward kernel that reads gf and f."""
import numpy as np


def rot_dst(rot, u, v, P):
    """Where element (u, v) of a plane lands under the clockwise rotation by rot * 90 degrees (elem.hip)."""
    if rot == 0:
        return u, v
    if rot == 1:
        return P - 1 - v, u
    if rot == 2:
        return P - 1 - u, P - 1 - v
    return v, P - 1 - u


def unrot_map(k, P):
    """-> (i, j, kept): [P, P] integer arrays, the position in f's plane of stack element (s, v), and kept[s, v] = False
    for the dropped row s = P-1 (whose i, j are meaningless)."""
    s, v = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    i, j = rot_dst((4 - k) & 3, s + 1, v, P)
    return i, j, s < P - 1


def zero_line(k, P):
    """Boolean [P, P]: the elements of f's plane that no stack element maps to (row 0 of the shifted plane)."""
    z = np.ones((P, P), dtype=bool)
    i, j, kept = unrot_map(k, P)
    z[i[kept], j[kept]] = False
    return z


def tile_stores(k, P, s0, v0):
    """The stores one lane of the Winograd output transform issues for its 2x2 tile at stack rows s0, s0+1, columns
    v0, v0+1 (csrc/wino.hip, UNROT): a list of (flat offset in f's plane, [values]) with values named ("o", r, c) for
    stack element (s0 + r, v0 + c) or 0 for the zero line.  Two pair stores; lanes of the top tile row add the zero
    line, lanes of the last one (whose second row Shift2d drops) store single elements."""
    rot, top, last = (4 - k) & 3, s0 == 0, s0 == P - 2
    o = lambda r, c: ("o", r, c)
    out = []
    if rot == 0:
        a = (s0 + 1) * P + v0
        out.append((a, [o(0, 0), o(0, 1)]))
        if not last:
            out.append((a + P, [o(1, 0), o(1, 1)]))
        if top:
            out.append((v0, [0, 0]))
    elif rot == 2:
        a = (P - 2 - s0) * P + (P - 2 - v0)
        out.append((a, [o(0, 1), o(0, 0)]))
        if not last:
            out.append((a - P, [o(1, 1), o(1, 0)]))
        if top:
            out.append(((P - 1) * P + (P - 2 - v0), [0, 0]))
    elif rot == 3:
        a = v0 * P + (P - 3 - s0)
        if not last:
            out += [(a, [o(1, 0), o(0, 0)]), (a + P, [o(1, 1), o(0, 1)])]
        if top:
            out += [(v0 * P + P - 1, [0]), (v0 * P + P - 1 + P, [0])]
        if last:
            out += [(v0 * P, [o(0, 0)]), (v0 * P + P, [o(0, 1)])]
    else:
        a = (P - 1 - v0) * P + s0 + 1
        if not last:
            out += [(a, [o(0, 0), o(1, 0)]), (a - P, [o(0, 1), o(1, 1)])]
        e = (P - 2 - v0) * P
        if top:
            out += [(e, [0]), (e + P, [0])]
        if last:
            out += [(e + P - 1, [o(0, 1)]), (e + P - 1 + P, [o(0, 0)])]
    return out
