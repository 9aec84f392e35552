"""ctypes binding of libkb2e.so (include/kb2e_engine.h).

This is the product path for Python callers (bench.py, tests): every call goes
through the C ABI into the HIP engine.  There is no CPU fallback -- if the
library or a GPU is missing, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KB2E_LIB") or os.path.join(HERE, "libkb2e.so")

MODELS = {"transe": 0, "transh": 1, "transr": 2, "E": 0, "H": 1, "R": 2}
STATUS = {0: "OK", 1: "EINVAL", 2: "EDEVICE", 3: "ESTATE", 4: "ENOMEM", 5: "EUNSUPPORTED", 6: "ESAMPLER"}
SAMPLER_GLIBC, SAMPLER_REPLAY = 0, 1
SCHEDULES = {"ordered": 0, "parallel": 1}

# Every symbol include/kb2e_engine.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "kb2e_default_config", "kb2e_create", "kb2e_destroy", "kb2e_last_error", "kb2e_upload_triples",
    "kb2e_init_params", "kb2e_transr_seed", "kb2e_upload_params", "kb2e_download_params", "kb2e_get_transr_work",
    "kb2e_set_transr_work", "kb2e_set_sample_stream", "kb2e_get_sample_stream", "kb2e_train_epoch", "kb2e_train_batches",
    "kb2e_synchronize", "kb2e_take_stats", "kb2e_rng_next", "kb2e_profile_enable", "kb2e_profile_query", "kb2e_counter",
    "kb2e_device_bytes", "kb2e_device_tables", "kb2e_renormalize", "kb2e_evaluate", "kb2e_evaluate_transr_compat",
    "kb2e_renormalize_rows", "kb2e_init_params_device", "kb2e_write_table", "kb2e_format_table",
    "kb2e_read_table", "kb2e_comm_unique_id", "kb2e_comm_init_rank", "kb2e_comm_init_group", "kb2e_merge_epoch",
    "kb2e_merge_epoch_group", "kb2e_comm_info", "kb2e_get_config", "kb2e_score_triples", "kb2e_predict",
    "kb2e_rank_triples", "kb2e_predict_relations", "kb2e_rank_relations", "kb2e_fit_thresholds",
    "kb2e_classify_triples", "kb2e_corrupt_triples", "kb2e_complete_triples", "kb2e_fold_in_entities",
    "kb2e_fold_in_relations", "kb2e_predict_joint", "kb2e_rank_joint", "kb2e_predict_path", "kb2e_rank_path",
    "kb2e_neighbors", "kb2e_score_candidates", "kb2e_rank_candidates",
]
COMM_ID_BYTES = 128
PATH_MAX_HOPS = 8  # KB2E_PATH_MAX_HOPS
READ_VERBATIM, READ_UNIT, READ_SHRINK = 0, 1, 2


class Config(C.Structure):
    _fields_ = [
        ("model", C.c_int32), ("dim", C.c_int32), ("num_entities", C.c_int32), ("num_relations", C.c_int32),
        ("learning_rate", C.c_double), ("margin", C.c_double), ("method", C.c_int32), ("distance", C.c_int32),
        ("num_batches", C.c_int32), ("seed", C.c_uint32), ("precision", C.c_int32), ("sampler", C.c_int32),
        ("transr_compat", C.c_int32), ("device", C.c_int32), ("schedule", C.c_int32), ("sub_batches", C.c_int32),
    ]


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"kb2e HIP engine not built: {LIB_PATH} missing (run `make`)")
        L = C.CDLL(LIB_PATH)
        vp, i32, i64, dp = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_double)
        i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        sig = {
            "kb2e_default_config": (None, [C.POINTER(Config)]),
            "kb2e_create": (i32, [C.POINTER(Config), C.POINTER(vp)]),
            "kb2e_get_config": (i32, [vp, C.POINTER(Config)]),
            "kb2e_destroy": (None, [vp]),
            "kb2e_last_error": (C.c_char_p, [vp]),
            "kb2e_upload_triples": (i32, [vp, i32p, i32p, i32p, i64]),
            "kb2e_init_params": (i32, [vp, dp, dp, dp]),
            "kb2e_init_params_device": (i32, [vp, dp, dp, dp, C.POINTER(i64)]),
            "kb2e_write_table": (i32, [vp, i32, C.c_char_p]),
            "kb2e_format_table": (i32, [vp, i32, C.c_char_p, i64, C.POINTER(i64)]),
            "kb2e_read_table": (i32, [vp, i32, C.c_char_p, i32]),
            "kb2e_upload_params": (i32, [vp, dp, dp, dp]),
            "kb2e_transr_seed": (i32, [vp, dp, dp]),
            "kb2e_download_params": (i32, [vp, dp, dp, dp]),
            "kb2e_get_transr_work": (i32, [vp, dp, dp]),
            "kb2e_set_transr_work": (i32, [vp, dp, dp]),
            "kb2e_set_sample_stream": (i32, [vp, i32p, i32p, u8p, i64]),
            "kb2e_get_sample_stream": (i32, [vp, i32p, i32p, u8p, i64]),
            "kb2e_train_epoch": (i32, [vp, dp, C.POINTER(i64)]),
            "kb2e_train_batches": (i32, [vp, i32]),
            "kb2e_synchronize": (i32, [vp]),
            "kb2e_take_stats": (i32, [vp, dp, C.POINTER(i64)]),
            "kb2e_rng_next": (i32, [vp]),
            "kb2e_profile_enable": (i32, [vp, i32]),
            "kb2e_profile_query": (i32, [vp, C.c_char_p, dp, C.POINTER(i64)]),
            "kb2e_device_bytes": (i64, [vp]),
            "kb2e_counter": (i32, [vp, C.c_char_p, C.POINTER(i64)]),
            "kb2e_device_tables": (i32, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i64),
                                         C.POINTER(i64), C.POINTER(i64)]),
            "kb2e_renormalize": (i32, [vp, u8p, u8p, u8p]),
            "kb2e_renormalize_rows": (i32, [vp, i32, i64, i64, vp]),
            "kb2e_evaluate": (i32, [vp, i32p, i32p, i32p, i64, i32p, i32p, i32p, i64, dp]),
            "kb2e_evaluate_transr_compat": (i32, [vp, i32p, i32p, i32p, i64, i32p, i32p, i32p, i64, dp, dp, vp,
                                                  vp]),
            "kb2e_score_triples": (i32, [vp, i32p, i32p, i32p, i64, dp]),
            "kb2e_predict": (i32, [vp, i32p, i32p, i32p, i64, i32, i32p, i32p, i32p, i64, i32p, dp, i32p]),
            "kb2e_rank_triples": (i32, [vp, i32p, i32p, i32p, i64, i32p, i32p, i32p, i64, C.POINTER(i64)]),
            "kb2e_predict_relations": (i32, [vp, i32p, i32p, i64, i32, i32p, i32p, i32p, i64, i32p, dp, i32p]),
            "kb2e_rank_relations": (i32, [vp, i32p, i32p, i32p, i64, i32p, i32p, i32p, i64, C.POINTER(i64)]),
            "kb2e_predict_joint": (i32, [vp, C.POINTER(i64), i32p, i32p, i32p, i64, i32, i32p, i32p, i32p, i64, i32p, dp,
                                         i32p]),
            "kb2e_rank_joint": (i32, [vp, C.POINTER(i64), i32p, i32p, i32p, i32p, i64, i32p, i32p, i32p, i64,
                                      C.POINTER(i64)]),
            "kb2e_predict_path": (i32, [vp, i32p, C.POINTER(i64), i32p, i32p, i64, i32, i32, i32, i32p, i32p, i32p, i64,
                                        i32p, dp, i32p, i32p]),
            "kb2e_rank_path": (i32, [vp, i32p, C.POINTER(i64), i32p, i32p, i32p, i64, i32, i32, i32p, i32p, i32p, i64,
                                     C.POINTER(i64)]),
            "kb2e_fit_thresholds": (i32, [vp, i32p, i32p, i32p, u8p, i64, dp, C.POINTER(i64), dp, C.POINTER(i64)]),
            "kb2e_classify_triples": (i32, [vp, i32p, i32p, i32p, i64, dp, u8p, dp]),
            "kb2e_corrupt_triples": (i32, [vp, i32p, i32p, i32p, i64, i32p, i32p, i32p, i64, C.c_uint64, i32, i32,
                                           i32p, i32p, C.POINTER(i64)]),
            "kb2e_complete_triples": (i32, [vp, i32p, i64, i32, i32p, i32p, i32p, i64, i32, i32, i32p, i32p, dp,
                                            C.POINTER(i64)]),
            "kb2e_neighbors": (i32, [vp, i32p, i64, i32, i32, i32, i32p, dp, i32p]),
            "kb2e_score_candidates": (i32, [vp, i32p, i32p, i32p, i32p, i64, C.POINTER(i64), i32p, i64, dp]),
            "kb2e_rank_candidates": (i32, [vp, i32p, i32p, i32p, i32p, i32p, i64, C.POINTER(i64), i32p, i64, i32p, i32p,
                                           i32p, i64, C.POINTER(i64), C.POINTER(i64)]),
            "kb2e_fold_in_entities": (i32, [vp, i32p, i64, i32p, i32p, i32p, i64, i32p, i32p, i32p, i64, i32, C.c_uint64,
                                            i32, i32, dp, dp, dp, C.POINTER(i64)]),
            "kb2e_fold_in_relations": (i32, [vp, i32p, i64, i32p, i32p, i32p, i64, i32p, i32p, i32p, i64, i32, i64,
                                             C.c_uint64, i32, i32, dp, dp, dp, dp, dp, C.POINTER(i64)]),
            "kb2e_comm_unique_id": (i32, [u8p]),
            "kb2e_comm_init_rank": (i32, [vp, i32, i32, u8p]),
            "kb2e_comm_init_group": (i32, [C.POINTER(vp), i32]),
            "kb2e_merge_epoch": (i32, [vp]),
            "kb2e_merge_epoch_group": (i32, [C.POINTER(vp), i32]),
            "kb2e_comm_info": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(i64)]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


class EngineError(RuntimeError):
    pass


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class Engine:
    """One training context on one GPU (the drop-in for Trainer::bfgs)."""

    def __init__(self, model, dim, num_entities, num_relations, *, rate=0.001, margin=1.0, method=1,
                 distance=0, batches=100, seed=0, precision=64, sampler=SAMPLER_GLIBC, transr_compat=True,
                 device=0, schedule="ordered", sub_batches=None):
        self.kind = MODELS[model] if isinstance(model, str) else int(model)
        self.n, self.ne, self.nr = dim, num_entities, num_relations
        cfg = Config()
        lib().kb2e_default_config(C.byref(cfg))
        cfg.model, cfg.dim, cfg.num_entities, cfg.num_relations = self.kind, dim, num_entities, num_relations
        cfg.learning_rate, cfg.margin, cfg.method, cfg.distance = rate, margin, method, distance
        cfg.num_batches, cfg.seed, cfg.precision, cfg.sampler = batches, seed, precision, sampler
        cfg.transr_compat, cfg.device = int(transr_compat), device
        cfg.schedule = SCHEDULES[schedule] if isinstance(schedule, str) else int(schedule)
        if sub_batches is not None:  # (None: the engine's default by width, kb2e_default_config)
            cfg.sub_batches = int(sub_batches)
        h = C.c_void_p()
        st = lib().kb2e_create(C.byref(cfg), C.byref(h))
        if st != 0:
            raise EngineError(f"kb2e_create failed: {STATUS.get(st, st)}")
        self.h = h
        self.cfg = Config()  # the context's own, defaults resolved (kb2e_get_config)
        self._check(lib().kb2e_get_config(self.h, C.byref(self.cfg)), "kb2e_get_config")

    def _check(self, st, what):
        if st != 0:
            msg = lib().kb2e_last_error(self.h)
            raise EngineError(f"{what}: {STATUS.get(st, st)}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "h", None):
            lib().kb2e_destroy(self.h)
            self.h = None

    __del__ = close

    def wshape(self):
        return {0: None, 1: (self.nr, self.n), 2: (self.nr, self.n, self.n)}[self.kind]

    def upload_triples(self, triples):
        t = np.ascontiguousarray(triples, dtype=np.int32)
        cols = [np.ascontiguousarray(t[:, k]) for k in range(3)]
        self._check(lib().kb2e_upload_triples(self.h, _ip(cols[0]), _ip(cols[1]), _ip(cols[2]), len(t)),
                    "upload_triples")

    def init_params(self):
        ent = np.zeros((self.ne, self.n))
        rel = np.zeros((self.nr, self.n))
        w = np.zeros(self.wshape()) if self.wshape() else None
        self._check(lib().kb2e_init_params(self.h, _dp(ent), _dp(rel), _dp(w)), "init_params")
        return ent, rel, w

    def init_params_device(self, fetch=True):
        """Trainer::prepTrain's draws made on the device (same values, same rng
        position); returns (ent, rel, w, near_ties), the tables None if not fetched."""
        ties = C.c_int64(0)
        if not fetch:
            self._check(lib().kb2e_init_params_device(self.h, None, None, None, C.byref(ties)), "init_params_device")
            return None, None, None, ties.value
        ent = np.zeros((self.ne, self.n))
        rel = np.zeros((self.nr, self.n))
        w = np.zeros(self.wshape()) if self.wshape() else None
        self._check(lib().kb2e_init_params_device(self.h, _dp(ent), _dp(rel), _dp(w), C.byref(ties)),
                    "init_params_device")
        return ent, rel, w, ties.value

    def write_table(self, table, path):
        """The device table (0 entities, 1 relations, 2 weights) as the reference's "%.6lf\\t" text file."""
        self._check(lib().kb2e_write_table(self.h, int(table), os.fsencode(path)), "write_table")

    def format_table(self, table):
        need = C.c_int64(0)
        lib().kb2e_format_table(self.h, int(table), None, 0, C.byref(need))
        buf = C.create_string_buffer(max(1, need.value))
        self._check(lib().kb2e_format_table(self.h, int(table), buf, need.value, C.byref(need)), "format_table")
        return buf.raw[:need.value]

    def read_table(self, table, path, mode=READ_VERBATIM):
        """Load a device table from "%lf" text (parsed on the device); mode: READ_VERBATIM / READ_UNIT / READ_SHRINK."""
        self._check(lib().kb2e_read_table(self.h, int(table), os.fsencode(path), int(mode)), "read_table")

    def transr_seed(self, ent, rel):
        ent = np.ascontiguousarray(ent, dtype=np.float64)
        rel = np.ascontiguousarray(rel, dtype=np.float64)
        self._check(lib().kb2e_transr_seed(self.h, _dp(ent), _dp(rel)), "transr_seed")

    def upload_params(self, ent, rel, w=None):
        ent = np.ascontiguousarray(ent, dtype=np.float64)
        rel = np.ascontiguousarray(rel, dtype=np.float64)
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        self._check(lib().kb2e_upload_params(self.h, _dp(ent), _dp(rel), _dp(w)), "upload_params")

    def download_params(self):
        ent = np.zeros((self.ne, self.n))
        rel = np.zeros((self.nr, self.n))
        w = np.zeros(self.wshape()) if self.wshape() else None
        self._check(lib().kb2e_download_params(self.h, _dp(ent), _dp(rel), _dp(w)), "download_params")
        return ent, rel, w

    def transr_work(self):
        a, b = np.zeros(self.n), np.zeros(self.n)
        self._check(lib().kb2e_get_transr_work(self.h, _dp(a), _dp(b)), "get_transr_work")
        return a, b

    def set_transr_work(self, a, b):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        self._check(lib().kb2e_set_transr_work(self.h, _dp(a), _dp(b)), "set_transr_work")

    def set_sample_stream(self, si, sj, side):
        si = np.ascontiguousarray(si, dtype=np.int32)
        sj = np.ascontiguousarray(sj, dtype=np.int32)
        side = np.ascontiguousarray(side, dtype=np.uint8)
        self._keep = (si, sj, side)
        self._check(lib().kb2e_set_sample_stream(self.h, _ip(si), _ip(sj),
                                                 side.ctypes.data_as(C.POINTER(C.c_uint8)), len(si)),
                    "set_sample_stream")

    def sample_stream(self, count):
        si = np.zeros(count, np.int32)
        sj = np.zeros(count, np.int32)
        side = np.zeros(count, np.uint8)
        self._check(lib().kb2e_get_sample_stream(self.h, _ip(si), _ip(sj), side.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                 count), "get_sample_stream")
        return si, sj, side

    # ------------------------------------------------ multi-GPU epoch merge
    @staticmethod
    def comm_unique_id():
        """A fresh RCCL id (bytes) for kb2e_comm_init_rank; made on one rank, handed to all."""
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        st = lib().kb2e_comm_unique_id(buf)
        if st != 0:
            raise EngineError(f"kb2e_comm_unique_id failed: {STATUS.get(st, st)}")
        return bytes(buf)

    def comm_init_rank(self, nranks, rank, comm_id):
        """Join the RCCL communicator (collective); rank 0's tables are broadcast."""
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(comm_id))
        self._check(lib().kb2e_comm_init_rank(self.h, int(nranks), int(rank), buf), "comm_init_rank")

    def merge_epoch(self):
        """T <- renorm(T0 + sum_r (T_r - T0)) over the communicator (collective)."""
        self._check(lib().kb2e_merge_epoch(self.h), "merge_epoch")

    def comm_info(self):
        n, r = C.c_int32(), C.c_int32()
        lo, cnt = C.c_int64(), C.c_int64()
        self._check(lib().kb2e_comm_info(self.h, C.byref(n), C.byref(r), C.byref(lo), C.byref(cnt)), "comm_info")
        return n.value, r.value, lo.value, cnt.value

    def train_epoch(self):
        loss = C.c_double(0)
        act = C.c_int64(0)
        self._check(lib().kb2e_train_epoch(self.h, C.byref(loss), C.byref(act)), "train_epoch")
        return loss.value, act.value

    def train_batches(self, nb):
        self._check(lib().kb2e_train_batches(self.h, int(nb)), "train_batches")

    def synchronize(self):
        self._check(lib().kb2e_synchronize(self.h), "synchronize")

    def take_stats(self):
        loss = C.c_double(0)
        act = C.c_int64(0)
        self._check(lib().kb2e_take_stats(self.h, C.byref(loss), C.byref(act)), "take_stats")
        return loss.value, act.value

    def rng_next(self):
        return lib().kb2e_rng_next(self.h)

    def profile(self, on=True):
        """on: False/0 off, True/1 every batch, P > 1 every P-th batch."""
        self._check(lib().kb2e_profile_enable(self.h, int(on)), "profile_enable")

    def profile_query(self, name):
        ms = C.c_double(0)
        n = C.c_int64(0)
        self._check(lib().kb2e_profile_query(self.h, name.encode(), C.byref(ms), C.byref(n)), "profile_query")
        return ms.value, n.value

    def counter(self, name):
        """A device-side schedule counter (include/kb2e_engine.h kb2e_counter)."""
        v = C.c_int64(0)
        self._check(lib().kb2e_counter(self.h, name.encode(), C.byref(v)), "counter")
        return v.value

    def renormalize(self, ent_rows=None, rel_rows=None, w_rows=None):
        keep = [None if m is None else np.ascontiguousarray(m, dtype=np.uint8) for m in (ent_rows, rel_rows, w_rows)]
        ptrs = [None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint8)) for m in keep]
        self._check(lib().kb2e_renormalize(self.h, *ptrs), "renormalize")

    def renormalize_rows(self, table, first, count, device_mask_ptr=None):
        """Norm constraint on rows [first, first + count) of table 0/1/2, mask in device memory."""
        self._check(lib().kb2e_renormalize_rows(self.h, int(table), int(first), int(count), device_mask_ptr),
                    "renormalize_rows")

    def evaluate(self, test, filt):
        """Link prediction (raw/filtered mean rank and hits@10) on the device tables."""
        test = np.ascontiguousarray(test, dtype=np.int32)
        filt = np.ascontiguousarray(filt, dtype=np.int32)
        tc = [np.ascontiguousarray(test[:, k]) for k in range(3)]
        fc = [np.ascontiguousarray(filt[:, k]) for k in range(3)]
        out = np.zeros(4)
        self._check(lib().kb2e_evaluate(self.h, _ip(tc[0]), _ip(tc[1]), _ip(tc[2]), len(test), _ip(fc[0]),
                                        _ip(fc[1]), _ip(fc[2]), len(filt), _dp(out)), "evaluate")
        return {"raw_rank": out[0], "raw_hits10": out[1], "filtered_rank": out[2], "filtered_hits10": out[3]}

    def evaluate_transr_compat(self, test, filt, work=None):
        """TransR link prediction with the reference evalTransR's accumulating
        energy work vectors; returns the ranks plus "ties" and the final "work"."""
        test = np.ascontiguousarray(test, dtype=np.int32)
        filt = np.ascontiguousarray(filt, dtype=np.int32)
        tc = [np.ascontiguousarray(test[:, k]) for k in range(3)]
        fc = [np.ascontiguousarray(filt[:, k]) for k in range(3)]
        w = np.zeros(2 * self.n) if work is None else np.ascontiguousarray(work, dtype=np.float64).reshape(-1).copy()
        out = np.zeros(5)
        self._check(lib().kb2e_evaluate_transr_compat(self.h, _ip(tc[0]), _ip(tc[1]), _ip(tc[2]), len(test),
                                                      _ip(fc[0]), _ip(fc[1]), _ip(fc[2]), len(filt), _dp(w),
                                                      _dp(out), None, None), "evaluate_transr_compat")
        return {"raw_rank": out[0], "raw_hits10": out[1], "filtered_rank": out[2], "filtered_hits10": out[3],
                "ties": int(out[4]), "work": w.reshape(2, self.n)}

    # ------------------------------------------------ using a trained model
    @staticmethod
    def _filter_cols(filt):
        if filt is None or len(filt) == 0:
            return [None, None, None], 0
        filt = np.ascontiguousarray(filt, dtype=np.int32)
        cols = [np.ascontiguousarray(filt[:, k]) for k in range(3)]
        return cols, len(filt)

    def score(self, triples):
        """Energy of each (head, tail, relation) row: float64[count], the reference's
        tripleEnergy bit for bit (TransR from zeroed work vectors)."""
        t = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
        cols = [np.ascontiguousarray(t[:, k]) for k in range(3)]
        out = np.zeros(len(t))
        self._check(lib().kb2e_score_triples(self.h, _ip(cols[0]), _ip(cols[1]), _ip(cols[2]), len(t), _dp(out)),
                    "score_triples")
        return out

    def predict(self, entities, relations, side, k, filt=None):
        """Top-k candidates of one-sided queries: side 1 asks for the tails of
        (entity, ?, relation), side 0 for the heads of (?, entity, relation);
        candidates whose triple is a row of `filt` are excluded.  Returns
        (ids int32[nq, k], energy float64[nq, k], found int32[nq]): ascending
        (energy, id), padded with -1 / +inf after found[q]."""
        e = np.ascontiguousarray(entities, dtype=np.int32).reshape(-1)
        r = np.ascontiguousarray(relations, dtype=np.int32).reshape(-1)
        s = np.ascontiguousarray(side, dtype=np.int32).reshape(-1)
        if not (len(e) == len(r) == len(s)):
            raise ValueError("entities, relations and side differ in length")
        nq, k = len(e), int(k)
        fc, nf = self._filter_cols(filt)
        kk = max(k, 1)
        ids = np.full((nq, kk), -1, np.int32)
        en = np.full((nq, kk), np.inf)
        found = np.zeros(nq, np.int32)
        self._check(lib().kb2e_predict(self.h, _ip(e), _ip(r), _ip(s), nq, k, *[None if c is None else _ip(c) for c in fc],
                                       nf, _ip(ids), _dp(en), _ip(found)), "predict")
        return ids, en, found

    def rank_triples(self, test, filt):
        """evaluate()'s ranks per test triple, in the caller's order: int64[ntest, 4] =
        head raw, head filtered, tail raw, tail filtered."""
        test = np.ascontiguousarray(test, dtype=np.int32)
        tc = [np.ascontiguousarray(test[:, k]) for k in range(3)]
        fc, nf = self._filter_cols(filt)
        ranks = np.zeros((len(test), 4), np.int64)
        self._check(lib().kb2e_rank_triples(self.h, _ip(tc[0]), _ip(tc[1]), _ip(tc[2]), len(test),
                                            *[None if c is None else _ip(c) for c in fc], nf,
                                            ranks.ctypes.data_as(C.POINTER(C.c_int64))), "rank_triples")
        return ranks

    def predict_relations(self, heads, tails, k, filt=None):
        """Top-k relations of (head, ?, tail) pairs: the candidates of pair q are the
        triples (heads[q], tails[q], r) of every relation r; those that are a row of
        `filt` are excluded.  Returns (ids int32[nq, k], energy float64[nq, k],
        found int32[nq]): ascending (energy, relation id), padded with -1 / +inf
        after found[q] (0 when every relation of the pair is known)."""
        h = np.ascontiguousarray(heads, dtype=np.int32).reshape(-1)
        t = np.ascontiguousarray(tails, dtype=np.int32).reshape(-1)
        if len(h) != len(t):
            raise ValueError("heads and tails differ in length")
        nq, k = len(h), int(k)
        fc, nf = self._filter_cols(filt)
        kk = max(k, 1)
        ids = np.full((nq, kk), -1, np.int32)
        en = np.full((nq, kk), np.inf)
        found = np.zeros(nq, np.int32)
        self._check(lib().kb2e_predict_relations(self.h, _ip(h), _ip(t), nq, k,
                                                 *[None if c is None else _ip(c) for c in fc], nf, _ip(ids), _dp(en),
                                                 _ip(found)), "predict_relations")
        return ids, en, found

    def rank_relations(self, test, filt):
        """The rank of each test triple's relation among all relations of its
        (head, tail) pair, in the caller's order: int64[ntest, 2] = raw, filtered."""
        test = np.ascontiguousarray(test, dtype=np.int32).reshape(-1, 3)
        tc = [np.ascontiguousarray(test[:, k]) for k in range(3)]
        fc, nf = self._filter_cols(filt)
        ranks = np.zeros((len(test), 2), np.int64)
        self._check(lib().kb2e_rank_relations(self.h, _ip(tc[0]), _ip(tc[1]), _ip(tc[2]), len(test),
                                              *[None if c is None else _ip(c) for c in fc], nf,
                                              ranks.ctypes.data_as(C.POINTER(C.c_int64))), "rank_relations")
        return ranks

    # ------------------------------------------------ conjunctive queries
    @staticmethod
    def _joint_arrays(queries):
        """offsets int64[nq + 1] and the (entity, relation, side) columns of the
        queries' rows, concatenated in order."""
        rows = [np.ascontiguousarray(q, dtype=np.int32).reshape(-1, 3) for q in queries]
        offsets = np.zeros(len(rows) + 1, np.int64)
        if rows:
            offsets[1:] = np.cumsum([len(r) for r in rows])
        cat = np.concatenate(rows + [np.zeros((0, 3), np.int32)])
        cols = [np.ascontiguousarray(cat[:, c]) for c in range(3)]
        return offsets, cols

    def predict_joint(self, queries, k, filt=None):
        """Top-k entities that fit several patterns at once.  `queries` is a
        sequence of int arrays [m_q, 3] of (entity, relation, side) rows, predict()'s
        patterns, 1 <= m_q <= 64; a candidate's joint energy is the sum of its
        energies over the query's rows, added in the given order, and it is
        excluded iff every one of its triples is a row of `filt`.  Returns (ids
        int32[nq, k], energy float64[nq, k], found int32[nq]) as predict()."""
        offsets, cols = self._joint_arrays(queries)
        nq, k = len(offsets) - 1, int(k)
        fc, nf = self._filter_cols(filt)
        kk = max(k, 1)
        ids = np.full((nq, kk), -1, np.int32)
        en = np.full((nq, kk), np.inf)
        found = np.zeros(nq, np.int32)
        self._check(lib().kb2e_predict_joint(self.h, offsets.ctypes.data_as(C.POINTER(C.c_int64)), _ip(cols[0]),
                                             _ip(cols[1]), _ip(cols[2]), nq, k,
                                             *[None if c is None else _ip(c) for c in fc], nf, _ip(ids), _dp(en),
                                             _ip(found)), "predict_joint")
        return ids, en, found

    def rank_joint(self, queries, truth, filt):
        """The rank of truth[q] among all entities by the joint energy of query q
        (predict_joint's queries), in the caller's order: int64[nq, 2] = raw, and
        with the excluded candidates other than the truth left out."""
        offsets, cols = self._joint_arrays(queries)
        nq = len(offsets) - 1
        tr = np.ascontiguousarray(truth, dtype=np.int32).reshape(-1)
        if len(tr) != nq:
            raise ValueError("queries and truth differ in length")
        fc, nf = self._filter_cols(filt)
        ranks = np.zeros((nq, 2), np.int64)
        self._check(lib().kb2e_rank_joint(self.h, offsets.ctypes.data_as(C.POINTER(C.c_int64)), _ip(cols[0]),
                                          _ip(cols[1]), _ip(cols[2]), _ip(tr), nq,
                                          *[None if c is None else _ip(c) for c in fc], nf,
                                          ranks.ctypes.data_as(C.POINTER(C.c_int64))), "rank_joint")
        return ranks

    # ------------------------------------------------ path queries
    @staticmethod
    def _path_arrays(anchors, paths):
        """anchors int32[nq], offsets int64[nq + 1] and the (relation, side) columns
        of the paths' hops, concatenated in order."""
        an = np.ascontiguousarray(anchors, dtype=np.int32).reshape(-1)
        hops = [np.ascontiguousarray(p, dtype=np.int32).reshape(-1, 2) for p in paths]
        if len(hops) != len(an):
            raise ValueError("anchors and paths differ in length")
        offsets = np.zeros(len(hops) + 1, np.int64)
        if hops:
            offsets[1:] = np.cumsum([len(h) for h in hops])
        cat = np.concatenate(hops + [np.zeros((0, 2), np.int32)])
        return an, offsets, np.ascontiguousarray(cat[:, 0]), np.ascontiguousarray(cat[:, 1])

    def predict_path(self, anchors, paths, k, filt=None, *, beam=0, no_loops=False, via=False):
        """Top-k entities at the end of a relation path.  Query q starts at
        anchors[q] and walks paths[q] = [[relation, side], ...], 1..8 hops in
        predict()'s convention (side 1: head -> tail, side 0: backwards).  An
        answer's energy is the smallest sum of hop energies, added in hop order,
        over the paths that end in it; after every hop but the last only the
        `beam` entities of smallest (energy, id) are walked on (0: all, the exact
        minimum).  no_loops: a hop may not stay on its entity.  An answer is
        excluded iff the rows of `filt` themselves lead to it along the path.
        Returns (ids int32[nq, k], energy float64[nq, k], found int32[nq]) as
        predict(); with via=True also int32[nq, k, 7], the intermediate entities
        of each answer's winning path, -1 behind."""
        an, offsets, rel, side = self._path_arrays(anchors, paths)
        nq, k = len(an), int(k)
        fc, nf = self._filter_cols(filt)
        kk = max(k, 1)
        ids = np.full((nq, kk), -1, np.int32)
        en = np.full((nq, kk), np.inf)
        found = np.zeros(nq, np.int32)
        w = np.full((nq, kk, PATH_MAX_HOPS - 1), -1, np.int32) if via else None
        self._check(lib().kb2e_predict_path(self.h, _ip(an), offsets.ctypes.data_as(C.POINTER(C.c_int64)), _ip(rel),
                                            _ip(side), nq, k, int(beam), int(no_loops),
                                            *[None if c is None else _ip(c) for c in fc], nf, _ip(ids), _dp(en),
                                            _ip(found), None if w is None else _ip(w)), "predict_path")
        return (ids, en, found, w) if via else (ids, en, found)

    def rank_path(self, anchors, paths, truth, filt=None, *, beam=0, no_loops=False):
        """The rank of truth[q] among all entities by the path energy of query q
        (predict_path's queries), in the caller's order: int64[nq, 2] = raw, and
        with the excluded candidates other than the truth left out."""
        an, offsets, rel, side = self._path_arrays(anchors, paths)
        nq = len(an)
        tr = np.ascontiguousarray(truth, dtype=np.int32).reshape(-1)
        if len(tr) != nq:
            raise ValueError("queries and truth differ in length")
        fc, nf = self._filter_cols(filt)
        ranks = np.zeros((nq, 2), np.int64)
        self._check(lib().kb2e_rank_path(self.h, _ip(an), offsets.ctypes.data_as(C.POINTER(C.c_int64)), _ip(rel),
                                         _ip(side), _ip(tr), nq, int(beam), int(no_loops),
                                         *[None if c is None else _ip(c) for c in fc], nf,
                                         ranks.ctypes.data_as(C.POINTER(C.c_int64))), "rank_path")
        return ranks

    # ------------------------------------------------ triple classification
    def fit_thresholds(self, triples, labels):
        """Per-relation energy thresholds fitted on labelled (head, tail, relation)
        rows (label 1: the triple holds, 0: it does not); a triple is positive iff
        energy <= threshold.  Returns (thresholds float64[R], counts int64[R, 3] =
        positives, negatives, correctly classified per relation, global_threshold,
        global_correct); a relation without a labelled triple gets the global
        threshold and counts 0 (the rule: include/kb2e_engine.h)."""
        t = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
        lab = np.ascontiguousarray(labels).reshape(-1)
        if len(lab) != len(t):
            raise ValueError("triples and labels differ in length")
        if len(lab) and (lab.min() < 0 or lab.max() > 255):
            raise EngineError("fit_thresholds: EINVAL: a label is neither 0 nor 1")
        lab = np.ascontiguousarray(lab, dtype=np.uint8)
        cols = [np.ascontiguousarray(t[:, k]) for k in range(3)]
        thr = np.zeros(self.nr)
        counts = np.zeros((self.nr, 3), np.int64)
        gthr, gcorrect = C.c_double(0), C.c_int64(0)
        self._check(lib().kb2e_fit_thresholds(self.h, _ip(cols[0]), _ip(cols[1]), _ip(cols[2]),
                                              lab.ctypes.data_as(C.POINTER(C.c_uint8)), len(t), _dp(thr),
                                              counts.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(gthr),
                                              C.byref(gcorrect)), "fit_thresholds")
        return thr, counts, gthr.value, gcorrect.value

    def classify(self, triples, thresholds, with_energy=False):
        """labels uint8[count]: 1 where energy <= thresholds[relation] (float64[R],
        +-inf allowed); with_energy=True also returns the energies (score()'s bits)."""
        t = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
        thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        if len(thr) != self.nr:
            raise EngineError(f"classify: EINVAL: {len(thr)} thresholds for {self.nr} relations")
        cols = [np.ascontiguousarray(t[:, k]) for k in range(3)]
        out = np.zeros(len(t), np.uint8)
        en = np.zeros(len(t)) if with_energy else None
        self._check(lib().kb2e_classify_triples(self.h, _ip(cols[0]), _ip(cols[1]), _ip(cols[2]), len(t), _dp(thr),
                                                out.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(en)), "classify_triples")
        return (out, en) if with_energy else out

    def corrupt(self, triples, known, seed=0, side=2, constrained=True):
        """One negative per row of `triples`: the head (side 0), the tail (side 1) or
        one of them by a fair coin (side 2) replaced, drawn from the entities seen
        in that slot of that relation among the rows of `known` (constrained, then
        from all entities), never equal to the replaced entity and never a row of
        `known`.  Returns (negatives int32[count, 3], failed): a row is (-1, -1,
        relation) where every draw was rejected.  The stream is a function of
        (seed, row index) alone (include/kb2e_engine.h kb2e_corrupt_triples)."""
        t = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
        cols = [np.ascontiguousarray(t[:, k]) for k in range(3)]
        kc, nk = self._filter_cols(known)
        nh = np.full(len(t), -1, np.int32)
        nt = np.full(len(t), -1, np.int32)
        failed = C.c_int64(0)
        self._check(lib().kb2e_corrupt_triples(self.h, _ip(cols[0]), _ip(cols[1]), _ip(cols[2]), len(t),
                                               *[None if c is None else _ip(c) for c in kc], nk,
                                               C.c_uint64(int(seed) & (2 ** 64 - 1)), int(side), int(bool(constrained)),
                                               _ip(nh), _ip(nt), C.byref(failed)), "corrupt_triples")
        return np.stack([nh, nt, cols[2]], axis=1), failed.value

    # ------------------------------------------------ knowledge-base completion
    def complete(self, relations, k, known=None, constrained=False, exclude_loops=False):
        """The k most plausible new triples of each listed relation: the candidates
        of relations[q] are the triples (h, t, relations[q]) of every entity pair
        (constrained: h from the relation's head pool, t from its tail pool, the
        entities seen in that slot among the rows of `known`); rows of `known` are
        excluded, and with exclude_loops the pairs h == t.  Returns (heads
        int32[nrel, k], tails int32[nrel, k], energy float64[nrel, k], found
        int64[nrel]): ascending (energy, head, tail), energies are score()'s bits,
        padded with -1 / -1 / +inf after found[q]."""
        r = np.ascontiguousarray(relations, dtype=np.int32).reshape(-1)
        nrel, k = len(r), int(k)
        for name, flag in (("constrained", constrained), ("exclude_loops", exclude_loops)):
            if flag not in (0, 1, False, True):
                raise EngineError(f"complete_triples: EINVAL: {name} must be 0 or 1")
        kc, nk = self._filter_cols(known)
        kk = max(k, 1)
        heads = np.full((nrel, kk), -1, np.int32)
        tails = np.full((nrel, kk), -1, np.int32)
        en = np.full((nrel, kk), np.inf)
        found = np.zeros(nrel, np.int64)
        self._check(lib().kb2e_complete_triples(self.h, _ip(r), nrel, k, *[None if c is None else _ip(c) for c in kc], nk,
                                                int(constrained), int(exclude_loops), _ip(heads), _ip(tails), _dp(en),
                                                found.ctypes.data_as(C.POINTER(C.c_int64))), "complete_triples")
        return heads, tails, en, found

    # ------------------------------------------------ entity neighbours
    def neighbors(self, entities, k, relation=-1, include_self=False):
        """The k nearest entities of each listed entity, in the entity space
        (relation -1: the rows of the entity table) or in relation r's space (the
        evaluator's projection for r).  The distance is the context's norm of
        P(x) - P(a), L1 or squared L2, in score()'s bits for (a, x, r) with a zero
        relation vector; the entity itself is a candidate only with include_self.
        1 <= k <= 128.  Returns (ids int32[nq, k], dist float64[nq, k], found
        int32[nq]): ascending (distance, id), padded with -1 / +inf after found[q]."""
        e = np.ascontiguousarray(entities, dtype=np.int32).reshape(-1)
        nq, k = len(e), int(k)
        if include_self not in (0, 1, False, True):
            raise EngineError("neighbors: EINVAL: include_self must be 0 or 1")
        kk = max(k, 1)
        ids = np.full((nq, kk), -1, np.int32)
        dist = np.full((nq, kk), np.inf)
        found = np.zeros(nq, np.int32)
        self._check(lib().kb2e_neighbors(self.h, _ip(e), nq, int(relation), k, int(include_self), _ip(ids), _dp(dist),
                                         _ip(found)), "neighbors")
        return ids, dist, found

    def knn_graph(self, k, relation=-1):
        """neighbors() of every entity, itself left out: row a lists a's k nearest."""
        return self.neighbors(np.arange(self.ne, dtype=np.int32), k, relation=relation)

    # ------------------------------------------------ candidate lists
    @staticmethod
    def _candidate_lists(candidates):
        """A sequence of id arrays as (offsets int64[nlists + 1], flat int32)."""
        arrs = [np.ascontiguousarray(c, dtype=np.int32).reshape(-1) for c in candidates]
        off = np.zeros(len(arrs) + 1, np.int64)
        if arrs:
            off[1:] = np.cumsum([len(a) for a in arrs])
        flat = np.concatenate(arrs) if arrs else np.zeros(0, np.int32)
        return off, np.ascontiguousarray(flat, dtype=np.int32)

    def _candidate_query(self, entities, relations, side, lists):
        e = np.ascontiguousarray(entities, dtype=np.int32).reshape(-1)
        r = np.ascontiguousarray(relations, dtype=np.int32).reshape(-1)
        s = np.ascontiguousarray(side, dtype=np.int32).reshape(-1)
        if not (len(e) == len(r) == len(s)):
            raise ValueError("entities, relations and side differ in length")
        li = None
        if lists is not None:
            li = np.ascontiguousarray(lists, dtype=np.int32).reshape(-1)
            if len(li) != len(e):
                raise ValueError("lists and entities differ in length")
        return e, r, s, li

    def score_candidates(self, entities, relations, side, candidates, lists=None):
        """Energies of one-sided queries against given candidate lists: query q is
        (entities[q], relations[q], side[q]) as predict()'s and is scored against
        the list candidates[lists[q]] (lists None: candidates[q]); a listing x is
        the triple (e, x, r) for side 1 and (x, e, r) for side 0, in score()'s
        bits.  A list that many queries name is uploaded once.  Returns one
        float64 array per query, in its list's order."""
        e, r, s, li = self._candidate_query(entities, relations, side, lists)
        off, flat = self._candidate_lists(candidates)
        nq, nl = len(e), len(off) - 1
        lens = np.diff(off)
        which = np.arange(nq) if li is None else li
        ok = nl > 0 and nq > 0 and (li is not None or nl == nq) and which.min(initial=0) >= 0 and which.max(initial=0) < nl
        total = int(lens[which].sum()) if ok else 0
        out = np.zeros(max(total, 1))
        self._check(lib().kb2e_score_candidates(self.h, _ip(e), _ip(r), _ip(s), None if li is None else _ip(li), nq,
                                                off.ctypes.data_as(C.POINTER(C.c_int64)), _ip(flat), nl, _dp(out)),
                    "score_candidates")
        cuts = np.cumsum(lens[which])[:-1]
        return np.split(out[:total], cuts)

    def rank_candidates(self, entities, relations, side, truth, candidates, filt=None, lists=None):
        """Rank truth[q] among the listings of query q's list (see
        score_candidates): ranks int64[nq, 2] = 1 + the listings other than the
        truth of strictly smaller energy, raw and with the listings whose triple is
        a row of `filt` left out; counted int64[nq, 2] = the listings that took
        part in each.  Returns (ranks, counted)."""
        e, r, s, li = self._candidate_query(entities, relations, side, lists)
        t = np.ascontiguousarray(truth, dtype=np.int32).reshape(-1)
        if len(t) != len(e):
            raise ValueError("truth and entities differ in length")
        off, flat = self._candidate_lists(candidates)
        nq, nl = len(e), len(off) - 1
        fc, nf = self._filter_cols(filt)
        ranks = np.zeros((max(nq, 1), 2), np.int64)
        counted = np.zeros((max(nq, 1), 2), np.int64)
        i64p = C.POINTER(C.c_int64)
        self._check(lib().kb2e_rank_candidates(self.h, _ip(e), _ip(r), _ip(s), _ip(t), None if li is None else _ip(li), nq,
                                               off.ctypes.data_as(i64p), _ip(flat), nl,
                                               *[None if c is None else _ip(c) for c in fc], nf,
                                               ranks.ctypes.data_as(i64p), counted.ctypes.data_as(i64p)),
                    "rank_candidates")
        return ranks[:nq], counted[:nq]

    def rerank(self, entities, relations, side, candidates, k, lists=None):
        """score_candidates() sorted on the host: per query the k listings of
        smallest (energy, entity id, position in the list).  Returns per query
        (ids int32[m], energy float64[m], position int64[m]), m = min(k, listings)."""
        e, r, s, li = self._candidate_query(entities, relations, side, lists)
        arrs = [np.ascontiguousarray(c, dtype=np.int32).reshape(-1) for c in candidates]
        en = self.score_candidates(e, r, s, arrs, lists=li)
        out = []
        for q, eq in enumerate(en):
            ids = arrs[q if li is None else li[q]]
            pos = np.arange(len(ids), dtype=np.int64)
            order = np.lexsort((pos, ids, eq))[:max(int(k), 0)]
            out.append((ids[order], eq[order], pos[order]))
        return out

    # ------------------------------------------------ entity fold-in
    def fold_in(self, free, examples, known=None, *, epochs, seed=0, side=2, max_sweeps=0, rows=None):
        """Learn the rows of the `free` entities from the (head, tail, relation)
        rows of `examples`, each of which holds exactly one free entity, with every
        other row, relation vector, normal and matrix frozen: `epochs` passes of
        margin-ranking SGD per free entity over its examples in the given order,
        negatives drawn per sample (side 0 head, 1 tail, 2 a coin) from the
        entities that are neither free nor make a row of `known` or `examples`.
        `rows` float64[nfree, dim] are the rows to start from (None: as they stand
        in the table); max_sweeps caps the coupling loops (0: 10000).  Only the
        free rows of the device entity table change.  Returns (rows
        float64[nfree, dim] as stored, loss float64[nfree, 2] = first and last
        pass, counts int64[nfree, 3] = active, failed, capped); the step is
        spelled out in include/kb2e_engine.h (kb2e_fold_in_entities)."""
        f = np.ascontiguousarray(free, dtype=np.int32).reshape(-1)
        ex = np.ascontiguousarray(examples, dtype=np.int32).reshape(-1, 3)
        ec = [np.ascontiguousarray(ex[:, k]) for k in range(3)]
        kc, nk = self._filter_cols(known)
        rin = None
        if rows is not None:
            rin = np.ascontiguousarray(rows, dtype=np.float64)
            if rin.shape != (len(f), self.n):
                raise ValueError(f"rows must be [{len(f)}, {self.n}]")
        out = np.zeros((len(f), self.n))
        loss = np.zeros((len(f), 2))
        counts = np.zeros((len(f), 3), np.int64)
        self._check(lib().kb2e_fold_in_entities(self.h, _ip(f), len(f), *[_ip(c) if len(ex) else None for c in ec],
                                                len(ex), *[None if c is None else _ip(c) for c in kc], nk, int(epochs),
                                                C.c_uint64(int(seed) & (2 ** 64 - 1)), int(side), int(max_sweeps),
                                                _dp(rin), _dp(out), _dp(loss),
                                                counts.ctypes.data_as(C.POINTER(C.c_int64))), "fold_in_entities")
        return out, loss, counts

    # ------------------------------------------------ relation fold-in
    def fold_in_relations(self, free, examples, known=None, *, epochs, batch_size=1, seed=0, side=2, max_sweeps=0,
                          rel=None, w=None):
        """Learn the parameters of the `free` relations -- their rows of the
        relation table, for TransH also their normals, for TransR also their
        matrices -- from the (head, tail, relation) rows of `examples`, whose
        relations must all be free, with every entity row and every other
        relation frozen: `epochs` passes per free relation over its examples in
        the given order, cut into batches of `batch_size` samples (the
        reference's batch rule: every gradient of a batch is taken at the
        parameters the batch found, the updates are applied in sample order);
        negatives drawn per sample (side 0 head, 1 tail, 2 a coin) from the
        entities that do not make a row of `known` or `examples`.  `rel`
        float64[nfree, dim] and `w` float64[nfree, dim] / [nfree, dim, dim] are
        the parameters to start from (None: as they stand in the tables);
        max_sweeps caps the coupling loops (0: 10000).  Returns (rel_rows
        float64[nfree, dim] as stored, w_rows likewise or None for TransE, loss
        float64[nfree, 2] = first and last pass, counts int64[nfree, 3] = active,
        failed, capped); the batch is spelled out in include/kb2e_engine.h
        (kb2e_fold_in_relations)."""
        f = np.ascontiguousarray(free, dtype=np.int32).reshape(-1)
        ex = np.ascontiguousarray(examples, dtype=np.int32).reshape(-1, 3)
        ec = [np.ascontiguousarray(ex[:, k]) for k in range(3)]
        kc, nk = self._filter_cols(known)
        wshape = {0: None, 1: (len(f), self.n), 2: (len(f), self.n, self.n)}[self.kind]
        rin = win = None
        if rel is not None:
            rin = np.ascontiguousarray(rel, dtype=np.float64)
            if rin.shape != (len(f), self.n):
                raise ValueError(f"rel must be [{len(f)}, {self.n}]")
        if w is not None:
            win = np.ascontiguousarray(w, dtype=np.float64)
            if wshape is not None and win.shape != wshape:
                raise ValueError(f"w must be {list(wshape)}")
        out = np.zeros((len(f), self.n))
        wout = None if wshape is None else np.zeros(wshape)
        loss = np.zeros((len(f), 2))
        counts = np.zeros((len(f), 3), np.int64)
        self._check(lib().kb2e_fold_in_relations(self.h, _ip(f), len(f), *[_ip(c) if len(ex) else None for c in ec],
                                                 len(ex), *[None if c is None else _ip(c) for c in kc], nk, int(epochs),
                                                 int(batch_size), C.c_uint64(int(seed) & (2 ** 64 - 1)), int(side),
                                                 int(max_sweeps), _dp(rin), _dp(win), _dp(out), _dp(wout), _dp(loss),
                                                 counts.ctypes.data_as(C.POINTER(C.c_int64))), "fold_in_relations")
        return out, wout, loss, counts

    def device_bytes(self):
        return lib().kb2e_device_bytes(self.h)


def _handles(engines):
    arr = (C.c_void_p * len(engines))(*[e.h for e in engines])
    return arr


def comm_init_group(engines):
    """One host thread driving every engine (kb2e_comm_init_group): RCCL over the
    engines' devices, or the local kernel backend when they share a device."""
    st = lib().kb2e_comm_init_group(_handles(engines), len(engines))
    if st != 0:
        raise EngineError(f"comm_init_group: {STATUS.get(st, st)}: {lib().kb2e_last_error(engines[0].h).decode()}")


def merge_epoch_group(engines):
    st = lib().kb2e_merge_epoch_group(_handles(engines), len(engines))
    if st != 0:
        raise EngineError(f"merge_epoch_group: {STATUS.get(st, st)}: {lib().kb2e_last_error(engines[0].h).decode()}")
