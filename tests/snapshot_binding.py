"""Binding of the env-snapshot entries (snap_*) of tests/emu/libjaco_emu*.so -- TEST INFRASTRUCTURE ONLY.

The host build of the env-snapshot table and its save / load routines (tests/emu/emu_driver.cpp over mujoco_jaco_amd/csrc/snapshot.h, the
header the GPU kernels of jaco_save_envs / jaco_load_envs are compiled from), in the emulator library of each layout (emu_binding.lib).
SnapHost wraps a set of per-env numpy arrays (an EmuJacoEnv's, or synthetic ones) as the "handle".
"""
import ctypes

import numpy as np

import emu_binding

_typed = set()


def lib(layout=""):
    L = emu_binding.lib(layout)
    if layout not in _typed:
        ip, up, vpp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_void_p)
        L.snap_field_name.restype = ctypes.c_char_p
        L.snap_field_name.argtypes = [ctypes.c_int]
        L.snap_bad_flag.restype = ctypes.c_uint
        L.snap_table.argtypes = [ctypes.c_int] * 4 + [ip, ip, up]
        L.snap_save.argtypes = [vpp] + [ctypes.c_int] * 5 + [ip, ctypes.c_int, up]
        L.snap_load.argtypes = [vpp] + [ctypes.c_int] * 5 + [ip, ctypes.c_int, up, ctypes.c_int, ip]
        L.snap_save.restype = L.snap_load.restype = None
        L.snap_task_floats, L.snap_cache_floats = L.emu_task_floats, L.emu_cache_floats   # (JTASK_N / JCACHE_N: one entry each in the library)
        _typed.add(layout)
    return L


def fields(layout=""):
    L = lib(layout)
    return [L.snap_field_name(i).decode() for i in range(L.snap_nfield())]


def table(nq, nv, nsensor, task_id, layout=""):
    """(W, {field: (words, offset)}, fingerprint) of the row for a model of these widths."""
    L = lib(layout)
    n = L.snap_nfield()
    words, off, fp = (ctypes.c_int * n)(), (ctypes.c_int * n)(), ctypes.c_uint()
    W = L.snap_table(nq, nv, nsensor, task_id, words, off, ctypes.byref(fp))
    return W, {f: (words[i], off[i]) for i, f in enumerate(fields(layout))}, fp.value


class SnapHost:
    """The host-side "handle": `arrays` {field name: [nenv, words] 32-bit numpy array}, fields not given are absent (NULL)."""

    def __init__(self, arrays, nq, nv, nsensor, task_id, nenv, layout=""):
        self.L, self.layout, self.dims, self.nenv = lib(layout), layout, (nq, nv, nsensor, task_id), nenv
        self.W, self.tab, self.fingerprint = table(nq, nv, nsensor, task_id, layout)
        self.arrays = dict(arrays)
        for f, a in self.arrays.items():
            assert a.dtype.itemsize == 4 and a.flags.c_contiguous and a.size == nenv * self.tab[f][0], (f, a.shape, a.dtype)

    def _ptrs(self, leave_out=()):
        P = (ctypes.c_void_p * len(self.tab))()
        for i, f in enumerate(self.tab):
            P[i] = self.arrays[f].ctypes.data if f in self.arrays and f not in leave_out else None
        return P

    @staticmethod
    def _idx(a):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, np.int32)
        return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))

    def save(self, envs=None, rows=None):
        e, ep = self._idx(envs)
        n = self.nenv if e is None else len(e)
        if rows is None:
            rows = np.zeros((n, self.W), np.uint32)
        self.L.snap_save(self._ptrs(), *self.dims, self.nenv, ep, n, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)))
        return rows

    def load(self, rows, envs=None, row_index=None, leave_out=(), nrows=None):
        e, ep = self._idx(envs)
        r, rp = self._idx(row_index)
        n = len(e) if e is not None else (len(r) if r is not None else self.nenv)
        self.L.snap_load(self._ptrs(leave_out), *self.dims, self.nenv, ep, n, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)),
                         len(rows) if nrows is None else nrows, rp)


def emu_arrays(e):
    """The per-env arrays of an EmuJacoEnv under their table names (the terminal latch lives inside the emulator library: wrapped in place)."""
    a = {"qpos": e.qpos, "qvel": e.qvel, "qacc_ws": e.qacc_ws, "sensordata": e.sensordata, "flags": e.flags, "stats": e.stats, "task": e.task,
         "cache": e.cache, "marker": e.marker}
    t = e.L.emu_last_terminal()
    if t:   # (sized by the first launch)
        a["terminal"] = np.ctypeslib.as_array(t, shape=(e.nenv, 2))
    return a


def emu_host(e):
    return SnapHost(emu_arrays(e), e.nq, e.nv, e.ns, e.task_id, e.nenv)
