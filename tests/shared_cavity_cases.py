"""What tests/test_gpu_shared_cavity.py builds its tables from: members drawn like parity_support.random_cfg, their device arrays
as views of one allocation per kind, the concatenation of a cavity's members into one system for the oracle, and the count of
the kernel nodes of a captured evaluation.  Importing this module touches no GPU."""
import ctypes
import re

import numpy as np
import torch

from parity_support import random_cfg

PRM = {"omegac": 0.0091, "couplstr": 1e-3, "phmass": 1.0}
L_TYPEID = 2
GUARD = 4                 # rows of 32 bytes before and after every force array
GUARD_VALUE = -7.25


def member_cfg(n, seed, photon_at=None, L=(31.0, 17.5, 23.25), image_range=3, photon_charge=0.0):
    """random_cfg; a member without a photon has no L-typed particle at all"""
    return random_cfg(n, seed, photon_at=photon_at, L=L, image_range=image_range, photon_charge=photon_charge)


class Table:
    """Members (cfg, cavity, is_carrier) on the device: positions, charges, images and guarded NaN-filled force arrays, each kind
    one allocation."""

    def __init__(self, members, capi, params=None):
        import cavitymd
        self.capi = capi
        self.cfgs = [m[0] for m in members]
        self.cavity = [int(m[1]) for m in members]
        self.is_carrier = [bool(m[2]) for m in members]
        self.n = [len(c["charge"]) for c in self.cfgs]
        self.start = np.concatenate([[0], np.cumsum(self.n)]).astype(np.int64)
        total = max(int(self.start[-1]), 1)
        pos = np.zeros((total, 4))
        chg = np.zeros(total)
        img = np.zeros((total, 3), dtype=np.int32)
        for k, c in enumerate(self.cfgs):
            a, b = int(self.start[k]), int(self.start[k + 1])
            pos[a:b, :3] = c["position"]
            pos[a:b, 3] = cavitymd.state.type_tag_as_double(c["typeid"])
            chg[a:b] = c["charge"]
            img[a:b] = c["image"]
        self.pos, self.chg, self.img = torch.from_numpy(pos).cuda(), torch.from_numpy(chg).cuda(), torch.from_numpy(img).cuda()
        self.fstart = self.start + GUARD * (2 * np.arange(len(self.start)) + 1)
        self.store = torch.full((total + 2 * GUARD * len(self.cfgs) + GUARD, 4), GUARD_VALUE, dtype=torch.float64, device="cuda")
        self.store2 = self.store.clone()                  # a second set, for the object compared against
        self.prm = params or [capi.make_params(PRM["omegac"], PRM["couplstr"], PRM["phmass"])] * (max(self.cavity) + 1)
        self.poison()

    def frc(self, k, store=None):
        a = int(self.fstart[k])
        return (self.store if store is None else store)[a:a + self.n[k]]

    def poison(self):
        for k in range(len(self.cfgs)):
            self.frc(k).fill_(float("nan"))
            self.frc(k, self.store2).fill_(float("nan"))

    def guards_intact(self):
        g = self.store.cpu().numpy()
        keep = np.ones(len(g), dtype=bool)
        for k in range(len(self.cfgs)):
            keep[int(self.fstart[k]):int(self.fstart[k]) + self.n[k]] = False
        return bool(np.all(g[keep] == GUARD_VALUE))

    def _ptrs(self, k, store=None):
        a = int(self.start[k])
        if self.n[k] == 0:
            return 0, 0, 0, 0
        return (self.pos[a:].data_ptr(), self.chg[a:].data_ptr(), self.img[a:].data_ptr(), self.frc(k, store).data_ptr())

    def item(self, k, cavity=None):
        c = self.cavity[k] if cavity is None else cavity
        box = tuple(float(x) for x in self.cfgs[k]["box"])
        return self.capi.shared_cavity_item(self.n[k], *self._ptrs(k), box, L_TYPEID if self.is_carrier[k] else -1, self.prm[c], c)

    def items(self):
        return [self.item(k) for k in range(len(self.cfgs))]

    def batch_item(self, k):
        """the same arrays as an item of cavmd_batch, the forces into the second set"""
        box = tuple(float(x) for x in self.cfgs[k]["box"])
        return self.capi.batch_item(self.n[k], *self._ptrs(k, self.store2), box, L_TYPEID if self.is_carrier[k] else -1,
                                    self.prm[self.cavity[k]])

    def forces(self, k, store=None):
        return self.frc(k, store).cpu().numpy()

    def members_of(self, cavity):
        return [k for k in range(len(self.cfgs)) if self.cavity[k] == cavity]

    def move(self, k, particle, delta):
        """adds `delta` to the position of one particle on the device and in the host copy"""
        self.cfgs[k]["position"][particle] += delta
        a = int(self.start[k]) + particle
        self.pos[a, :3] = torch.from_numpy(self.cfgs[k]["position"][particle]).cuda()


def concatenated(cfgs):
    """One system out of a cavity's members, in member order: positions pre-unwrapped, fl(p + img * L), with image 0 -- exactly
    what every evaluation computes first -- in a unit box.  Returns (cfg, the first particle of every member)."""
    start = np.concatenate([[0], np.cumsum([len(c["charge"]) for c in cfgs])]).astype(np.int64)
    pos = np.concatenate([c["position"] + c["image"] * np.asarray(c["box"]) for c in cfgs]).reshape(-1, 3)
    cfg = {"name": "cavity", "position": pos, "typeid": np.concatenate([c["typeid"] for c in cfgs]).astype(np.int32),
           "charge": np.concatenate([c["charge"] for c in cfgs]), "image": np.zeros((len(pos), 3), dtype=np.int32),
           "types": ["O", "N", "L"], "box": (1.0, 1.0, 1.0), "L_typeid": L_TYPEID, "params": dict(PRM)}
    return cfg, start


def block_equal(a, b, but=("sequence", "n_partials")):
    """two cavmd_result blocks byte-equal except the named fields"""
    a, b = bytearray(bytes(a)), bytearray(bytes(b))
    for name in but:
        f = getattr(type_of_result(), name)
        a[f.offset:f.offset + f.size] = b[f.offset:f.offset + f.size] = bytes(f.size)
    return a == b


def type_of_result():
    from cavitymd import _capi
    return _capi.Result


def _hip():
    """the HIP runtime this process has loaded (torch's)"""
    for line in open("/proc/self/maps"):
        m = re.search(r"(/\S*libamdhip64\.so\S*)", line)
        if m:
            return ctypes.CDLL(m.group(1))
    raise RuntimeError("no HIP runtime is loaded")


def captured_node_types(enqueue):
    """The node types (hipGraphNodeType: 0 = kernel) of the graph that `enqueue(stream handle)` gives when captured on a fresh
    stream; also what `enqueue` returned.  The graph is never instantiated."""
    hip = _hip()
    vp = ctypes.c_void_p
    hip.hipStreamBeginCapture.argtypes = [vp, ctypes.c_int]
    hip.hipStreamEndCapture.argtypes = [vp, ctypes.POINTER(vp)]
    hip.hipGraphGetNodes.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    hip.hipGraphDestroy.argtypes = [vp]
    stream = torch.cuda.Stream()
    stream.synchronize()
    graph = vp()
    assert hip.hipStreamBeginCapture(vp(stream.cuda_stream), 1) == 0          # hipStreamCaptureModeThreadLocal
    try:
        returned = enqueue(stream.cuda_stream)
    finally:
        assert hip.hipStreamEndCapture(vp(stream.cuda_stream), ctypes.byref(graph)) == 0
    n = ctypes.c_size_t()
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    nodes = (vp * max(n.value, 1))()
    assert hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) == 0
    types = []
    for i in range(n.value):
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(vp(nodes[i]), ctypes.byref(t)) == 0
        types.append(t.value)
    assert hip.hipGraphDestroy(graph) == 0
    return types, returned
