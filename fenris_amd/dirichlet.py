"""Dirichlet conditions on single displacement components (rollers, symmetry planes): the (nodes, masks) pairs that
fh_set_operator_dirichlet_dofs and fh_apply_dirichlet_dofs_* take.  A mask is one byte per node, bit j set = component j is constrained;
ALL_COMPONENTS (all ones) is what a node set stores.  Nothing here needs a device.

    op = MatrixFreeOperator(asm).with_dirichlet_dofs(face_x0, [0]).with_dirichlet_dofs(face_y0, [1])   # rollers on two planes
"""
import numpy as np

from . import _ffi

ALL_COMPONENTS = 0xFF


def dof_masks(nodes, components):
    """(nodes as uint64, masks as uint8) of one with_dirichlet_dofs call.  components: an (n, S) boolean array, one row per node, or a
    sequence of component indices applied to every listed node.  A row without a component and an index outside 0..7 are refused."""
    nodes = _ffi.as_u64(nodes).reshape(-1)
    comps = np.asarray(components)
    if comps.dtype == np.bool_:
        if comps.ndim != 2 or comps.shape[0] != len(nodes) or not 1 <= comps.shape[1] <= 8:
            raise ValueError("a boolean components array has one row per node and one column per solution component")
        masks = (comps.astype(np.uint8) << np.arange(comps.shape[1], dtype=np.uint8)).sum(axis=1).astype(np.uint8)
    else:
        if comps.ndim != 1 or comps.size == 0 or not np.issubdtype(comps.dtype, np.integer):
            raise ValueError("components is an (n, S) boolean array or a non-empty sequence of component indices")
        if comps.min() < 0 or comps.max() > 7:
            raise ValueError("a component index must lie in 0..7")
        masks = np.full(len(nodes), np.bitwise_or.reduce(np.uint8(1) << comps.astype(np.uint8)), dtype=np.uint8)
    if len(masks) and masks.min() == 0:
        raise ValueError("every listed node needs at least one constrained component")
    return nodes, masks


class DofSet:
    """A set of constrained dofs: sorted unique nodes (uint64) with the OR of the masks each was listed with (uint8)."""

    def __init__(self, nodes, masks):
        nodes = _ffi.as_u64(nodes).reshape(-1)
        masks = np.ascontiguousarray(masks, dtype=np.uint8).reshape(-1)
        if len(nodes) != len(masks):
            raise ValueError("one mask per node")
        self.nodes, inverse = np.unique(nodes, return_inverse=True)
        self.masks = np.zeros(len(self.nodes), dtype=np.uint8)
        np.bitwise_or.at(self.masks, inverse, masks)

    @staticmethod
    def of(held):
        """None, a node list (every component) or a DofSet, as a DofSet"""
        if isinstance(held, DofSet):
            return held
        nodes = _ffi.as_u64([] if held is None else held).reshape(-1)
        return DofSet(nodes, np.full(len(nodes), ALL_COMPONENTS, dtype=np.uint8))

    def joined(self, nodes, components):
        """this set and one more with_dirichlet_dofs call"""
        n, m = dof_masks(nodes, components)
        return DofSet(np.concatenate([self.nodes, n]), np.concatenate([self.masks, m]))

    def node_masks(self, num_nodes):
        """one mask byte per node of a mesh (0: free)"""
        out = np.zeros(int(num_nodes), dtype=np.uint8)
        out[self.nodes.astype(np.int64)] = self.masks
        return out

    def injected(self, inj, num_nodes):
        """the set of a coarse level whose node j is the fine node inj[j] (GeometricMultigrid carries the masks down the hierarchy)"""
        coarse = self.node_masks(num_nodes)[np.asarray(inj, dtype=np.int64)]
        keep = np.nonzero(coarse)[0]
        return DofSet(keep.astype(np.uint64), coarse[keep])

    def dof_indices(self, solution_dim):
        """the constrained dofs as indices S node + component, ascending (a mask of all ones: every component)"""
        s = int(solution_dim)
        held = (self.masks[:, None] >> np.arange(s, dtype=np.uint8)) & 1
        k, c = np.nonzero(held)
        return np.sort(self.nodes[k].astype(np.int64) * s + c)

    def key(self):
        return self.nodes.tobytes() + b"|" + self.masks.tobytes()

    def __len__(self):
        return len(self.nodes)


def with_dirichlet_dofs(obj, nodes, components):
    """the shared body of every with_dirichlet_dofs: the object's held set (obj._nodes: None, a node list or a DofSet) joined with this call"""
    obj._nodes = DofSet.of(obj._nodes).joined(nodes, components)
    obj._bind(force=True)
    return obj
