"""What tests/test_gpu_large_volumes.py and tests/ab/test_ab_large_volumes.py share: the huge pair of one shape of
tests/large_volume_cases.py on the device with the one engine alive on it, device-side slice reads of a prepared field, and ICGN3D1
solved on every block of a shape against the oracle on the crops.  Not a test module; imports HIP only when it is used."""
import ctypes

import numpy as np

import large_volume_cases as lv

GB = 10 ** 9


def voxels(key):
    dz, dy, dx = lv.SHAPES[key]
    return dz * dy * dx


# shape key -> (the target is the reference tensor, device bytes the case needs: the pair and ICGN3D1's five volumes on it)
CASES = {"INDEX31": (False, 7 * 4 * voxels("INDEX31") + GB), "SLAB": (False, 7 * 4 * voxels("SLAB") + GB), "REFUSED": (True, 4 * voxels("REFUSED") + GB)}
assert 61 * GB < CASES["INDEX31"][1] < 62 * GB and 69 * GB < CASES["SLAB"][1] < 70 * GB and 19 * GB < CASES["REFUSED"][1] < 20 * GB


class Huge:
    """The pair of one shape and the one engine that is alive on it."""

    def __init__(self, torch, key):
        self.key, self.torch = key, torch
        self.shape = lv.SHAPES[key]
        same = CASES[key][0]
        self.ref = torch.zeros(self.shape, dtype=torch.float32, device="cuda")     # (an allocation failure is an error, not a skip)
        self.tar = self.ref if same else torch.zeros(self.shape, dtype=torch.float32, device="cuda")
        for b in lv.BLOCKS[key]:
            for t, a in zip((self.ref,) if same else (self.ref, self.tar), lv.crop(b)):
                t[b.slices] = torch.from_numpy(np.array(a)).cuda()
        torch.cuda.synchronize()
        self.engine, self.tag = None, None

    def used(self):
        free, total = self.torch.cuda.mem_get_info()
        return total - free

    def get(self, tag, make, prepare=True):
        """the engine `tag`, made (and prepared) when another one held the device"""
        if self.tag != tag:
            self.drop()
            e = make()
            e.set_images(self.ref, self.tar)
            if prepare:
                e.prepare()
                e.synchronize()
                print("%s %s: %.2f GB of device memory in use after prepare()" % (self.key, tag, self.used() / GB))
            self.engine, self.tag = e, tag
        return self.engine

    def drop(self):
        if self.engine is not None:
            self.engine.close()
        self.engine, self.tag = None, None

    def close(self):
        self.drop()
        self.ref = self.tar = None


# ---- device-side slice reads ------------------------------------------------------------------------------------------------------
def read_block(e, name, block):
    """the field over the block, (bz, by, bx): one hipMemcpy2D per plane of the block, never the whole array"""
    from opencorr_amd import capi
    ptr, count = ctypes.c_void_p(), ctypes.c_size_t()
    capi.check(capi.lib().oc_hip_get_field(e._h, name.encode(), ctypes.byref(ptr), ctypes.byref(count)))
    e.synchronize()
    dz, dy, dx = block.shape
    assert count.value == dz * dy * dx
    out = np.empty(block.size, dtype=np.float32)
    copy2d = capi.hip_runtime().hipMemcpy2D          # (the one runtime of this process)
    copy2d.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
    copy2d.restype = ctypes.c_int
    for i in range(block.bz):
        src = ptr.value + 4 * (((block.z0 + i) * dy + block.y0) * dx + block.x0)
        status = copy2d(out[i].ctypes.data, out[i].strides[0], src, 4 * dx, 4 * block.bx, block.by, 2)    # hipMemcpyDeviceToHost
        assert status == 0, "hipMemcpy2D: %d" % status
    return out


# ---- the oracle on the crops, once ------------------------------------------------------------------------------------------------
_want = {}


def want(key, contract, guesses, radii):
    """(the queue of all blocks of the shape in volume coordinates, the oracle's records for it)"""
    k = (key, contract, guesses, radii)
    if k not in _want:
        qs, ws = [], []
        for b in lv.BLOCKS[key]:
            q, _ = lv.solver_queue(b, guesses, radii)
            qs.append(lv.shift(q, b))
            ws.append(lv.solve(contract, lv.prepared(b), q, radii))
        _want[k] = (np.concatenate(qs), np.concatenate(ws))
    return _want[k]


def solve_and_compare(e, key, contract, radii, what, calls=2):
    e.set_subset(*radii)
    for guesses in ("int", "half"):
        q, w = want(key, contract, guesses, radii)
        for call in range(calls):          # twice: the engine and its scratch are used again
            got = e.compute(q.copy())
            assert np.array_equal(lv.bits(got[:, :3]), lv.bits(q[:, :3]))
            lv.assert_same_but_xyz(got, w, "%s ICGN3D1 %s %s %s, %s guesses, call %d" % (key, radii, contract, what, guesses, call + 1))


def set_contract(e, contract):
    e.set_tuning("arith_fma", 1 if contract == "fma" else 0)
    e.set_tuning("arith_onepass3d", 1 if contract == "onepass" else 0)


def icgn3d1(eng, key):
    r = lv.RADII[key][0]
    return lambda: eng.ICGN3D1(r[0], r[1], r[2], lv.CONV, lv.STOP)
