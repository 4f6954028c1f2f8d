"""Host-side mirror of the reference's ``BpDecoder`` (src_python/ldpc/bp_decoder/_bp_decoder.pyx).

Same constructor keywords, property names, alias strings, exception types and messages as the
reference, so code written against ``ldpc.BpDecoder`` runs unchanged; the arithmetic happens in
libldpc_hip.so (HIP kernels for gfx950) behind ``ldpc_amd.engine.HipBpEngine``.  There is no CPU
fallback: ``decode`` raises if the HIP library or a GPU is missing.

Additions over the reference (it has no batch API): ``decode_batch`` and the
``*_batch`` result views.

Reference behaviours deliberately reproduced (each cited where implemented):
  * effective defaults come from the base initialiser's ``kwargs.get`` (pyx:90-100), not from the
    subclass signature: ``bp_method`` defaults to product_sum, ``max_iter=0`` means ``n``;
  * an all-zero input returns zeros with ``converge=True`` WITHOUT running BP, leaving
    ``log_prob_ratios`` / ``iter`` / ``decoding`` from the previous call (pyx:679-681, 688-690);
  * the output array has the input's dtype (pyx:673, 693-695).
"""
from __future__ import annotations

import warnings
from typing import List, Optional, Union

import numpy as np
import scipy.sparse

from ldpc_amd.helpers.scipy_helpers import convert_to_binary_sparse

# ldpc::bp enums (bp.hpp:23-38)
PRODUCT_SUM, MINIMUM_SUM = 0, 1
SERIAL, PARALLEL, SERIAL_RELATIVE = 0, 1, 2
SYNDROME, RECEIVED_VECTOR, AUTO = 0, 1, 2

_PS_ALIASES = ("prod_sum", "product_sum", "ps", "0", "prod sum")  # pyx:386
_MS_ALIASES = ("min_sum", "minimum_sum", "ms", "1", "minimum sum", "min sum")  # pyx:388
_UNSET = object()  # "keyword not passed by the caller"


def _bp_method_code(value) -> int:
    """The alias table of the ``bp_method`` setter (pyx:384-394) as a function."""
    key = str(value).lower()
    if key in _PS_ALIASES:
        return PRODUCT_SUM
    if key in _MS_ALIASES:
        return MINIMUM_SUM
    raise ValueError(f"BP method '{value}' is invalid. \
                    Please choose from the following methods: \
                    'product_sum', 'minimum_sum'")


_WAVE_RUNGS = ((4, 2), (4, 4), (6, 3), (8, 4), (8, 8), (16, 8))  # bp_wave_f32_kernel's instantiations (rows, columns): LDPC_WAVE_LADDER
_WAVE_F32_LDS_STATIC = 64  # ldpc_amd/csrc/bp_wave_f32_kernel.h: what plan_wave_f32 leaves free of a workgroup's 160 KiB for the kernel's static LDS


def float32_lane_node_takes(pcm, forced=False) -> bool:
    """Whether the lane = node float32 kernel (``BpDecoder.float32_lane_node``) takes the code -- the refusals of plan_wave_f32
    (ldpc_amd/csrc/host_onchip.h) restated without a GPU: rows of at most 16 entries and columns of at most 8; 16-bit positions and column
    numbers; padding every row to the rung's weight costs at most twice the entries plus 1024 (the default small-code kernel mode only:
    ``forced=True`` -- modes 1, 3, 4, 5 -- waives it); the shared tables and one syndrome's private region in its smaller form (FP32
    messages, the hard-decision words, the syndrome bytes; the log-ratios stored straight to memory) within 160 KiB - 64 of LDS.  It says
    nothing about the lane = edge families, which modes -1, 1 and 6 ask first."""
    h = scipy.sparse.csr_matrix(pcm)
    m, n = h.shape
    if m <= 0 or n <= 0 or h.nnz <= 0 or h.nnz * 16 >= (1 << 22):
        return False
    rows = int(np.diff(h.indptr).max())
    cmax = int(np.bincount(h.indices, minlength=n).max())
    rung = next(((r, c) for r, c in _WAVE_RUNGS if rows <= r and cmax <= c), None)
    if rung is None:
        return False
    dr, dc = rung
    mp, np_ = (m + 63) // 64 * 64, (n + 63) // 64 * 64
    rm = dr * mp
    if rm + 2 >= 65536 or np_ + 1 >= 65536 or (not forced and rm > 2 * h.nnz + 1024):
        return False
    up16 = lambda b: (b + 15) & ~15  # noqa: E731
    shared = up16(rm * 2 + dc * np_ * 2 + mp)
    private = up16((rm + 2) * 4 + (np_ // 64 + 1) * 8 + mp)
    return shared + private <= 160 * 1024 - _WAVE_F32_LDS_STATIC


def _check_pcm_type(pcm, spaces=12):
    if not isinstance(pcm, (np.ndarray, scipy.sparse.spmatrix)):  # pyx:17-21, 113-117
        # (the reference's message carries the indentation of its source line across a backslash continuation: 12 spaces in
        # BpDecoderBase.__cinit__, pyx:113-117, 8 in Py2BpSparse, pyx:17-21)
        raise TypeError("The input matrix is of an invalid type. Please input" + " " * spaces +
                        f"a np.ndarray or scipy.sparse.spmatrix object, not {type(pcm)}")


def _ingest(pcm) -> scipy.sparse.csr_matrix:
    """Py2BpSparse (pyx:9-49): validate and return canonical CSR (sorted columns, ones only)."""
    _check_pcm_type(pcm, spaces=8)
    # (a copy: the normalisation below must not reach into the caller's arrays -- the reference only reads pcm.nonzero();
    # like the reference's helper, convert_to_binary_sparse itself drops explicit zeros of a sparse input in place)
    h = scipy.sparse.csr_matrix(convert_to_binary_sparse(pcm), copy=True)
    h.sum_duplicates()  # insert_entry returns the existing entry for a repeated coordinate
    h.data[:] = 1       # (sparse_matrix_base.hpp:437-440), so duplicates collapse to a single one
    h.sort_indices()
    return h


def io_test(pcm):
    """Round-trip a matrix through the ingest path (reference ``io_test``, pyx:74-78)."""
    return scipy.sparse.csr_matrix(_ingest(pcm), dtype=np.uint8)


# ---- what Cython does with annotated arguments -------------------------------------------------------------------
# The reference's classes are Cython `cdef class`es compiled with annotation typing: an argument annotated with a builtin
# type (`value: int`, `input_type: str`, `Optional[float]`, `List[int]`) must be EXACTLY of that type (None allowed only for
# Optional[...]), `value: float` / `sigma: float` become C doubles (anything with __float__ / __index__ converts), `value: bool`
# becomes a C truth value, and a violation is a TypeError whose text is Cython's.  python_test/test_bp_decoder.py:143-168 pins
# some of these; tests/golden/api_reference.json (generated from the reference) pins all of them.
def _type_name(t) -> str:
    return t.__name__ if t.__module__ == "builtins" else f"{t.__module__}.{t.__name__}"


def _typed(name, value, typ, optional=True):
    """Exact-type test of an argument annotated with the builtin / extension type ``typ``."""
    if value is None and optional:
        return
    if type(value) is typ or (typ is np.ndarray and isinstance(value, np.ndarray)):
        return
    msg = f"Argument '{name}' has incorrect type (expected {_type_name(typ)}, got {_type_name(type(value))})"
    if isinstance(value, typ):
        msg += (". Note that Cython is deliberately stricter than PEP-484 and rejects subclasses of builtin types. If you need to "
                "pass subclasses then set the 'annotation_typing' directive to False.")
    raise TypeError(msg)


def _c_double(value) -> float:
    """Conversion of a Python object to a C double (``__pyx_PyFloat_AsDouble``)."""
    if isinstance(value, float):
        return float(value)
    t = type(value)
    if hasattr(t, "__float__") or hasattr(t, "__index__"):
        return float(value)
    raise TypeError(f"must be real number, not {t.__name__}")


def _readonly(name, owner):
    """Setter of a read-only property: the message of the reference's Cython getset descriptor."""
    def refuse(self, value):
        raise AttributeError(f"attribute '{name}' of 'ldpc.bp_decoder._bp_decoder.{owner}' objects is not writable")
    return refuse


class BpDecoderBase:
    """Parameter/validation surface shared by the BP decoder family (``cdef class BpDecoderBase``, pyx:82-579)."""

    def __init__(self, pcm, **kwargs):
        error_rate = kwargs.get("error_rate", None)  # pyx:90-100
        error_channel = kwargs.get("error_channel", None)
        max_iter = kwargs.get("max_iter", 0)
        bp_method = kwargs.get("bp_method", 0)
        ms_scaling_factor = kwargs.get("ms_scaling_factor", 1.0)
        schedule = kwargs.get("schedule", 0)
        omp_thread_count = kwargs.get("omp_thread_count", 1)
        random_serial_schedule = kwargs.get("random_serial_schedule", False)
        random_schedule_seed = kwargs.get("random_schedule_seed", 0)
        serial_schedule_order = kwargs.get("serial_schedule_order", None)
        channel_probs = kwargs.get("channel_probs", [None])

        self._engine = None
        self._engine_key = None
        self._device = kwargs.get("_device", -1)
        # additive: device_ids=[...] shards every decode_batch over those GPUs inside this process (ldpc_hip_bp_multi)
        self._device_ids = kwargs.get("device_ids", None)
        if self._device_ids is not None:
            self._device_ids = [int(d) for d in self._device_ids]
            if not self._device_ids or any(d < 0 for d in self._device_ids):
                raise ValueError("device_ids must be a non-empty list of GPU ordinals")
        # "cython": NumPy inputs go through the Cython binding of the C++ host class (ldpc_amd/bp_decoder/_bp_core.pyx,
        # the reference's own binding style); "ctypes": everything through ldpc_amd/engine.py.  Same C ABI underneath.
        self._backend = kwargs.get("_backend", None)
        self._cy = None
        self._message_dtype = "float64"
        self._engine_dtype = "float64"  # what the engine's handle is set to (a new handle starts at float64)
        self._memory = None             # memory_strength: None (off) or an (n,) float64 array
        self._engine_memory = None      # what the engine's handle is set to (a new handle starts with memory off)
        self._relay = None              # relay: None (off) or (strengths (legs, n), leg_iters (legs,), stop_after)
        self._engine_relay = None       # ... what the engine's handle is set to
        self._decimation = None         # decimation: None (off) or (round_iters, max_rounds, freeze_llr)
        self._engine_decimation = None  # ... what the engine's handle is set to
        self._float32_lane_node = False            # float32_lane_node: the lane = node route of the float32 message mode, opt-in
        self._engine_float32_lane_node = False     # ... what the engine's handle is set to
        self._decimation_lane_node = False         # decimation_lane_node: the lane = node route of guided decimation, opt-in
        self._engine_decimation_lane_node = False  # ... what the engine's handle is set to

        self._h = _ingest(pcm)
        self.m, self.n = int(pcm.shape[0]), int(pcm.shape[1])

        # state of the C++ object (`new BpDecoderCpp(...)`, pyx:132 / bp.hpp:77-132)
        self._channel_probs = np.zeros(self.n, np.float64)
        self._channel_dirty = True
        self._max_iter = 0
        self._bp_method = PRODUCT_SUM
        self._schedule = PARALLEL
        self._ms_scaling_factor = 1.0
        self._omp_thread_count = 1
        self._serial_schedule_order = np.arange(self.n, dtype=np.int64)  # bp.hpp:120-124
        self._random_schedule_seed = 0
        self._seed_epoch = 0
        self._random_serial_schedule = False
        self._bp_input_type = SYNDROME
        self._decoding = np.zeros(self.n, np.uint8)
        self._log_prob_ratios = np.zeros(self.n, np.float64)
        self._iterations = 0
        self._converge = False
        # batch views (additive API)
        self.converge_batch = None
        self.iter_batch = None
        self.log_prob_ratios_batch = None

        self.bp_method = bp_method  # pyx:135-142
        self.max_iter = max_iter
        self.ms_scaling_factor = ms_scaling_factor
        self.schedule = schedule
        self.serial_schedule_order = serial_schedule_order
        self.random_schedule_seed = random_schedule_seed
        self.omp_thread_count = omp_thread_count
        self.random_serial_schedule = random_serial_schedule

        if isinstance(channel_probs, (list, np.ndarray)):  # ldpc_v1 compatibility, pyx:145-147
            if len(channel_probs) > 0 and channel_probs[0] is not None:
                error_channel = channel_probs

        if error_channel is not None:
            self.error_channel = error_channel
        elif error_rate is not None:
            self.error_rate = error_rate
        else:  # pyx:153-155 (the reference forgets the f-prefix; the literal braces are its message)
            raise ValueError("Please specify the error channel. Either: 1) error_rate: float or 2) error_channel:\
            list of floats of length equal to the block length of the code {self.n}.")

    # ---- channel (pyx:167-233) ------------------------------------------------------------------
    @property
    def error_rate(self) -> np.ndarray:
        return self._channel_probs.astype(float).copy()

    @error_rate.setter
    def error_rate(self, value: Optional[float]) -> None:
        _typed("value", value, float)
        if value is not None:
            if not isinstance(value, float):
                raise ValueError("The `error_rate` parameter must be specified as a single float value.")
            self._channel_probs[:] = value
            self._channel_dirty = True

    @property
    def error_channel(self) -> np.ndarray:
        return self._channel_probs.astype(float).copy()

    @error_channel.setter
    def error_channel(self, value) -> None:
        if value is not None:
            if len(value) != self.n:
                raise ValueError(f"The error channel vector must have length {self.n}, not {len(value)}.")
            self._channel_dirty = True
            for i in range(self.n):  # element by element into the C++ vector (pyx:222-223): a bad element stops HERE
                self._channel_probs[i] = _c_double(value[i])

    def update_channel_probs(self, value) -> None:
        self.error_channel = value

    @property
    def channel_probs(self) -> np.ndarray:
        return self._channel_probs.astype(float).copy()

    channel_probs = channel_probs.setter(_readonly("channel_probs", "BpDecoderBase"))

    # ---- input vector type (pyx:236-276) --------------------------------------------------------
    @property
    def input_vector_type(self) -> str:
        return {SYNDROME: "syndrome", RECEIVED_VECTOR: "received_vector", AUTO: "auto"}[self._bp_input_type]

    @input_vector_type.setter
    def input_vector_type(self, input_type: str):
        _typed("input_type", input_type, str, optional=False)
        key = input_type.lower()
        if key in ("auto", "a", "2"):
            if self.m == self.n:
                raise ValueError("Please specify the input vector type. Either: 1) input_vector_type: 'syndrome' or 2) input_vector_type:\
                'received_vector'.")
            self._bp_input_type = AUTO
        elif key in ("syndrome", "s", "0"):
            self._bp_input_type = SYNDROME
        elif key in ("received_vector", "r", "1"):
            self._bp_input_type = RECEIVED_VECTOR
        else:
            raise ValueError(f"The input vector type '{input_type}' is invalid. \
                    Please choose from the following methods: \
                    'input_vector_type=syndrome', 'input_vector_type=received_vector'")

    # ---- results (pyx:279-329) ------------------------------------------------------------------
    @property
    def log_prob_ratios(self) -> np.ndarray:
        return np.array(self._log_prob_ratios, dtype=np.float64)

    @property
    def converge(self) -> bool:
        return bool(self._converge)

    @property
    def iter(self) -> int:
        return int(self._iterations)

    @property
    def check_count(self) -> int:
        return self.m

    @property
    def bit_count(self) -> int:
        return self.n

    log_prob_ratios = log_prob_ratios.setter(_readonly("log_prob_ratios", "BpDecoderBase"))
    converge = converge.setter(_readonly("converge", "BpDecoderBase"))
    iter = iter.setter(_readonly("iter", "BpDecoderBase"))
    check_count = check_count.setter(_readonly("check_count", "BpDecoderBase"))
    bit_count = bit_count.setter(_readonly("bit_count", "BpDecoderBase"))

    # ---- algorithm parameters (pyx:332-579) -----------------------------------------------------
    @property
    def max_iter(self) -> int:
        return self._max_iter

    @max_iter.setter
    def max_iter(self, value: int) -> None:
        _typed("value", value, int, optional=False)
        if not isinstance(value, int):
            raise ValueError("max_iter input parameter is invalid. This must be specified as a positive int.")
        if value < 0:
            raise ValueError(f"max_iter input parameter must be a positive int. Not {value}.")
        self._max_iter = value if value != 0 else self.n  # pyx:357

    @property
    def bp_method(self) -> str:
        return "product_sum" if self._bp_method == PRODUCT_SUM else "minimum_sum"

    @bp_method.setter
    def bp_method(self, value: Union[str, int]) -> None:
        self._bp_method = _bp_method_code(value)

    @property
    def schedule(self) -> str:
        return {PARALLEL: "parallel", SERIAL: "serial", SERIAL_RELATIVE: "serial_relative"}[self._schedule]

    @schedule.setter
    def schedule(self, value: Union[str, int]) -> None:
        key = str(value).lower()
        if key in ("parallel", "p", "0"):
            self._schedule = PARALLEL
        elif key in ("serial", "s", "1"):
            self._schedule = SERIAL
        elif key in ("serial_relative", "sr", "2"):
            self._schedule = SERIAL_RELATIVE
        else:
            raise ValueError(f"The BP schedule method '{value}' is invalid. \
                    Please choose from the following methods: \
                    'schedule=parallel', 'schedule=serial', 'schedule=serial_relative'")

    @property
    def serial_schedule_order(self):
        if self._serial_schedule_order is None or len(self._serial_schedule_order) == 0:
            return None
        return np.array(self._serial_schedule_order, dtype=int)

    @serial_schedule_order.setter
    def serial_schedule_order(self, value) -> None:
        if value is None:
            return
        if not len(value) == self.n:
            raise Exception("Input error. The `serial_schedule_order` input parameter must have length equal to the length of the code.")
        for i in range(self.n):
            if not isinstance(value[i], (int, np.int64, np.int32)) or value[i] < 0 or value[i] >= self.n:
                raise ValueError(f"serial_schedule_order[{i}] is invalid. It must be a non-negative integer less than {self.n}.")
        self._serial_schedule_order = np.asarray(value, dtype=np.int64).copy()
        self.random_serial_schedule = False

    @property
    def ms_scaling_factor(self) -> float:
        return self._ms_scaling_factor

    @ms_scaling_factor.setter
    def ms_scaling_factor(self, value: float) -> None:
        value = _c_double(value)
        if not isinstance(value, (float, int)):
            raise TypeError("The ms_scaling factor must be specified as a float")
        self._ms_scaling_factor = float(value)

    @property
    def omp_thread_count(self) -> int:
        if self._omp_thread_count != 1:
            warnings.warn("The OpenMP functionality is not yet implemented")
        return self._omp_thread_count

    @omp_thread_count.setter
    def omp_thread_count(self, value: int) -> None:
        _typed("value", value, int, optional=False)
        if not isinstance(value, int) or value < 1:
            raise TypeError("The omp_thread_count must be specified as a\
            positive integer.")
        self._omp_thread_count = value
        if self._omp_thread_count != 1:
            warnings.warn("The OpenMP functionality is not yet implemented")

    @property
    def random_schedule_seed(self) -> int:
        return self._random_schedule_seed

    @random_schedule_seed.setter
    def random_schedule_seed(self, value: int) -> None:
        _typed("value", value, int, optional=False)
        if not isinstance(value, int) or value < -2:
            raise ValueError("The value of random_schedule_seed must\
            be a positive integer. Set as -1 to disable to the random\
            schedule. Set as 0 to use the system clock.")
        self._random_serial_schedule = True  # pyx:551 (the constructor resets it right after, pyx:142)
        self._random_schedule_seed = value
        self._seed_epoch = getattr(self, "_seed_epoch", 0) + 1  # every call re-seeds the generator (bp.hpp:142-145)

    @property
    def random_serial_schedule(self) -> bool:
        return self._random_serial_schedule

    @random_serial_schedule.setter
    def random_serial_schedule(self, value: bool) -> None:
        self._random_serial_schedule = bool(value)  # a C truth value

    # ---- message precision (additive; not a constructor keyword: the signatures are the reference's) ----------
    @property
    def message_dtype(self) -> str:
        """``'float64'`` (default): the reference's arithmetic, bit for bit.  ``'float32'``: minimum-sum on the parallel schedule with FP32
        messages -- half the message traffic; decisions, flags, iteration counts and log-ratios are those of the FP32 restatement of the
        algorithm (every operation one FP32 operation, same order), NOT the reference's bits.  ``log_prob_ratios`` stay float64 (each an
        FP32 posterior widened).  With ``'float32'``, product-sum, the serial schedules, ``channel_probs=``, soft-syndrome decoding and
        ``device_ids=[...]`` raise ``NotImplementedError`` at decode time."""
        return self._message_dtype

    @message_dtype.setter
    def message_dtype(self, value) -> None:
        names = {"float64": "float64", "float32": "float32"}
        key = names.get(value) if isinstance(value, str) else ("float64" if value is np.float64 else "float32" if value is np.float32 else None)
        if key is None:
            raise ValueError(f"message_dtype must be 'float64', 'float32', np.float64 or np.float32, not {value!r}.")
        self._message_dtype = key

    @property
    def float32_lane_node(self) -> bool:
        """``False`` (default): with ``message_dtype='float32'`` only the codes of the two lane = edge kernel families are decoded on chip;
        every other code takes the per-pass kernels (four launches an iteration, the messages in HBM).  ``True``: a code beyond them -- rows
        of at most 16, columns of at most 8 entries, a syndrome's state within LDS (``ldpc_amd.bp_decoder.float32_lane_node_takes``) -- is
        decoded on chip by the lane = node kernel (``ldpc_hip_bp_set_f32_lane_node``).  The results are the same bits either way.  Setting it
        requires no particular ``message_dtype``; it is read only by float32 decodes."""
        return self._float32_lane_node

    @float32_lane_node.setter
    def float32_lane_node(self, value) -> None:
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError(f"float32_lane_node must be a bool, not {value!r}.")
        self._float32_lane_node = bool(value)

    @property
    def float32_route(self) -> str:
        """Which kernels a ``message_dtype='float32'`` decode takes on this decoder as it is set now, for a batch of the size last decoded
        (1 before any): ``HipBpEngine.f32_route`` -- ``"per_pass"``, ``"bp_edge"``, ``"bp_edge8"``, and with ``float32_lane_node`` also
        ``"bp_wave"`` / ``"bp_wave_team"`` (one wavefront / a team per syndrome).  It answers whatever ``message_dtype`` is."""
        if self._device_ids is not None:
            raise NotImplementedError("float32_route with device_ids=[...]: float32 messages are decoded on one GPU only.")
        return self._get_engine().f32_route(getattr(self, "_last_batch", 1))

    @property
    def row_prior_route(self) -> str:
        """Which kernels a ``decode_batch(..., channel_probs=P)`` takes on this decoder as it is set now, for a batch of the size last decoded
        (1 before any): ``HipBpEngine.row_prior_route`` -- ``"per_pass"``, ``"bp_edge"``, ``"bp_edge8"``, ``"bp_wave"`` / ``"bp_wave_team"``
        (the lane = node kernel with one wavefront / a team per syndrome) or ``"bp_small"`` (the slot kernel).  The routes give the same bits
        and differ by an order of magnitude in speed.  Where such a decode is refused -- a serial schedule, ``message_dtype='float32'``,
        ``memory_strength``, ``relay``, ``decimation``, ``device_ids=[...]`` -- its ``NotImplementedError`` is raised instead."""
        self._require_modes()  # (what any decode of this decoder is refused for speaks first, as in decode_batch)
        self._require_modes("channel_probs: per-row channel probabilities are decoded {only}")
        if self._schedule != PARALLEL:
            raise NotImplementedError(f"channel_probs with schedule='{self.schedule}': the serial schedules decode with the decoder's own "
                                      "channel probabilities only; per-row probabilities need schedule='parallel'.")
        if self._device_ids is not None:
            raise NotImplementedError("row_prior_route with device_ids=[...]: the rows of channel_probs are not sharded over several GPUs; "
                                      "decode on one GPU.")
        return self._get_engine().row_prior_route(getattr(self, "_last_batch", 1))

    # ---- memory min-sum BP (additive; not a constructor keyword either) ----------------------------------------
    @property
    def memory_strength(self):
        """``None`` (default): plain BP.  A float (every bit) or an array of ``n`` memory strengths, each finite and in ``[-1, 1)``: memory
        min-sum BP (Mem-BP; with per-bit strengths DMem-BP, the building block of Relay-BP) -- every iteration's bit pass takes
        ``(1 - gamma[j]) * prior[j] + gamma[j] * (bit j's previous posterior)`` for the prior of bit j; strength 0 on every bit is plain
        min-sum, bit for bit.  The getter returns ``None`` or a float64 array copy.  Minimum-sum, the parallel schedule and float64 messages
        on one GPU: with memory on, product-sum, the serial schedules, soft-syndrome decoding, ``message_dtype='float32'``,
        ``channel_probs=``, ``device_ids=[...]`` and a nonzero strength on a bit whose channel probability is 0 or 1 raise
        ``NotImplementedError`` at decode time.  The results are those of the NumPy restatement of the algorithm (tests/mem_bp_util.py),
        bit for bit."""
        return None if self._memory is None else self._memory.copy()

    @memory_strength.setter
    def memory_strength(self, value) -> None:
        if value is None:
            self._memory = None
            return
        try:
            g = np.array(value, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"memory_strength must be None, a float or an array of {self.n} floats, not {value!r}.") from None
        if g.ndim == 0:
            g = np.full(self.n, float(g), np.float64)
        if g.shape != (self.n,):
            raise ValueError(f"memory_strength must be None, a float or an array of length {self.n}, not of shape {g.shape}.")
        if not (np.isfinite(g).all() and (g >= -1.0).all() and (g < 1.0).all()):
            raise ValueError("memory_strength: every strength must be finite and in [-1, 1).")
        self._memory = g

    # ---- Relay-BP (additive; not a constructor keyword either) ---------------------------------------------------
    @property
    def relay(self):
        """``None`` (default): off.  Set to a dict of ``ldpc_amd.relay_decoder.relay_schedule`` keywords (``gamma0``, ``pre_iter``,
        ``num_sets``, ``set_max_iter``, ``gamma_dist_interval``, ``stop_nconv``, ``strengths``, ``seed``): every decode then runs Relay-BP
        (``ldpc_hip_bp_set_relay``) -- chained memory min-sum legs whose iteration limits take the place of ``max_iter``.
        Read back as ``(strengths, leg_iters, stop_after)``.  Minimum-sum, parallel schedule, float64 messages, one GPU, OSD_0 at most; not
        together with ``memory_strength``, ``channel_probs=`` or soft syndromes -- ``NotImplementedError`` at decode time."""
        return None if self._relay is None else (self._relay[0].copy(), self._relay[1].copy(), self._relay[2])

    @relay.setter
    def relay(self, value) -> None:
        if value is None:
            self._relay = None
            return
        if not isinstance(value, dict):
            raise ValueError(f"relay must be None or a dict of relay_schedule keywords, not {value!r}.")
        from ldpc_amd.relay_decoder import relay_schedule
        self._relay = relay_schedule(self.n, **value)

    @property
    def relay_route(self) -> str:
        """The kernel route the relay (or ``memory_strength``) decode takes on this decoder as it is set now, for the batch size last decoded
        through NumPy arrays (1 before any): ``HipBpEngine.relay_route`` -- ``"per_pass"`` is 10 - 60x slower than the other four.
        ``ValueError`` when neither ``relay`` nor ``memory_strength`` is set."""
        if self._relay is None and self._memory is None:
            raise ValueError("relay_route: neither relay nor memory_strength is set.")
        self._require_modes(message_dtype=False)
        return self._get_engine().relay_route(getattr(self, "_relay_batch", 1))

    # ---- BP with guided decimation (additive; not a constructor keyword either) -----------------------------------
    @property
    def decimation(self):
        """``None`` (default): off.  Set to a dict of ``ldpc_amd.bpgd_decoder.decimation_schedule`` keywords (``round_iters=5``,
        ``max_rounds=None`` -- n --, ``freeze_llr=25.0``): every decode then runs BP with guided decimation (``ldpc_hip_bp_set_decimation``;
        DESIGN.md section 7e) -- rounds of ``round_iters`` min-sum iterations, the most reliable bit frozen at ``+-freeze_llr`` after every
        round that ends unsolved, the messages kept; ``round_iters`` and ``max_rounds`` take the place of ``max_iter``.  Read back as such a
        dict.  Minimum-sum, parallel schedule, float64 messages, one GPU, OSD_0 at most, and a code the lane = edge kernels take -- or, with
        ``decimation_lane_node``, the lane = node kernel -- (``decimation_route``); not together with ``memory_strength``, ``relay``, ``channel_probs=`` or soft syndromes --
        ``NotImplementedError`` at decode time."""
        if self._decimation is None:
            return None
        return dict(round_iters=self._decimation[0], max_rounds=self._decimation[1], freeze_llr=self._decimation[2])

    @decimation.setter
    def decimation(self, value) -> None:
        if value is None:
            self._decimation = None
            return
        if not isinstance(value, dict):
            raise ValueError(f"decimation must be None or a dict of decimation_schedule keywords, not {value!r}.")
        from ldpc_amd.bpgd_decoder import decimation_schedule
        self._decimation = decimation_schedule(self.n, **value)

    @property
    def decimation_lane_node(self) -> bool:
        """``False`` (default): guided decimation runs on the lane = edge kernels only and refuses every other code.  ``True``: a code beyond
        them -- rows of at most 16, columns of at most 8 entries, a syndrome's state within LDS (``ldpc_amd.bpgd_decoder.lane_node_takes``)
        -- is decoded by the lane = node kernel (``ldpc_hip_bp_set_decimation_lane_node``).  Read only while ``decimation`` is set."""
        return self._decimation_lane_node

    @decimation_lane_node.setter
    def decimation_lane_node(self, value) -> None:
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError(f"decimation_lane_node must be a bool, not {value!r}.")
        self._decimation_lane_node = bool(value)

    def _no_decimation_kernel(self) -> bool:
        """No handle is needed to say that no kernel takes the code: neither lane = edge family, nor -- where asked for -- the lane = node kernel."""
        from ldpc_amd.bpgd_decoder import lane_edge_route, lane_node_takes
        return lane_edge_route(self._h) == "unavailable" and not (self._decimation_lane_node and lane_node_takes(self._h))

    @property
    def decimation_route(self) -> str:
        """Which kernels decode with guided decimation on this decoder as it is set now: ``HipBpEngine.decimation_route`` -- ``"bp_edge"``,
        ``"bp_edge8"``, with ``decimation_lane_node`` also ``"bp_wave"`` / ``"bp_wave_team"``, or ``"unavailable"`` (a code none of them
        takes).  ``ValueError`` when ``decimation`` is not set; where the decoder is
        set to something decimation cannot serve at all (product-sum, a serial schedule, float32 messages, several GPUs, ``memory_strength``
        or ``relay``) there is no route to name and the ``NotImplementedError`` of a decode is raised instead, with its reason."""
        if self._decimation is None:
            raise ValueError("decimation_route: decimation is not set.")
        if self._no_decimation_kernel():
            return "unavailable"
        self._require_modes(message_dtype=False)
        return self._get_engine().decimation_route(getattr(self, "_relay_batch", 1))

    # ---- what the four modes refuse, stated once (the C side's twin: ldpc_amd/csrc/mode_host.h) ---------------------------------------------
    # One row per mode, asked in this order; within a row the rules are asked in the order of _require_modes.  Where the modes differ the row
    # says so: ``random_serial`` -- whether random_serial_schedule alone breaks the schedule rule (float32 messages look at ``schedule`` only);
    # ``excludes`` -- the modes that must be off, each with its own sentence; ``strengths`` -- where a nonzero strength needs a probability
    # strictly between 0 and 1 (None: no such rule); ``route`` -- the mode needs a code the lane = edge kernels take.  ``only``: the mode's own
    # wording for the ``{only}`` of a caller's ``what``.  A new mode is a new row.
    _MODES = (
        dict(key="message_dtype='float32'", on=lambda d: d._message_dtype == "float32", off="message_dtype='float64'", name="float32 messages", plural=True,
             only="with float64 messages only", excludes=(), random_serial=False, float64_only=False, strengths=None, route=False,
             product_sum="its tanh / log have no bit-exact float32 form here; float32 messages are available for bp_method='minimum_sum' only."),
        dict(key="decimation", on=lambda d: d._decimation is not None, off="decimation=None", name="guided decimation", plural=False,
             only="without decimation only", random_serial=True, float64_only=True, strengths=None, route=True,
             excludes=(("memory_strength", lambda d: d._memory is not None, "the two exclude each other; set memory_strength=None or decimation=None."),
                       ("relay", lambda d: d._relay is not None, "the two exclude each other; set relay=None or decimation=None.")),
             product_sum="guided decimation is built on the minimum-sum kernels only."),
        dict(key="relay", on=lambda d: d._relay is not None, off="relay=None", name="Relay-BP", plural=False,
             only="without the relay only", random_serial=True, float64_only=True, strengths=lambda d: (d._relay[0] != 0.0).any(axis=0), every_leg=" in every leg", route=False,
             excludes=(("memory_strength", lambda d: d._memory is not None, "the relay's legs carry their own strengths; set memory_strength=None."),),
             product_sum="the memory strengths are defined for bp_method='minimum_sum' only."),
        dict(key="memory_strength", on=lambda d: d._memory is not None, off="memory_strength=None", name="memory min-sum", plural=False,
             only="without memory only", excludes=(), random_serial=True, float64_only=True, strengths=lambda d: d._memory != 0.0, every_leg="", route=False,
             product_sum="the memory strengths are defined for bp_method='minimum_sum' only."),
    )

    def _require_modes(self, what=None, message_dtype=True):
        """What the modes that are on cannot do is refused here, at decode time and before any handle is made, with its reason.  ``what``: the
        call's own addition, which no mode does -- its ``{only}`` takes each mode's own wording.  ``message_dtype=False``: the three variants
        alone (the route properties, which name no float32 route)."""
        for mode in self._MODES:
            if not mode["on"](self) or (mode is self._MODES[0] and not message_dtype):
                continue
            key, name = mode["key"], mode["name"]
            if what is not None:
                raise NotImplementedError(f"{key} with {what.format(only=mode['only'])}; set {mode['off']}.")
            for other, other_on, why in mode["excludes"]:
                if other_on(self):
                    raise NotImplementedError(f"{key} with {other}: {why}")
            if self._bp_method != MINIMUM_SUM:
                raise NotImplementedError(f"{key} with bp_method='product_sum': {mode['product_sum']}")
            random_serial = mode["random_serial"] and self._random_serial_schedule
            if self._schedule != PARALLEL or random_serial:
                raise NotImplementedError(f"{key} with schedule='{self.schedule}'{' and random_serial_schedule' if random_serial else ''}: "
                                          f"{name} need{'' if mode['plural'] else 's'} schedule='parallel'.")
            if mode["float64_only"] and self._message_dtype != "float64":
                raise NotImplementedError(f"{key} with message_dtype='float32': {name} is decoded with float64 messages only.")
            if self._device_ids is not None:
                raise NotImplementedError(f"{key} with device_ids=[...]: {name} {'are' if mode['plural'] else 'is'} not sharded over several GPUs; decode on one GPU.")
            if mode["strengths"] is not None:
                p = self._channel_probs
                bad = np.flatnonzero(mode["strengths"](self) & ~((p > 0.0) & (p < 1.0)))
                if len(bad):
                    raise NotImplementedError(f"{key}: bit {int(bad[0])} has a nonzero memory strength and a channel probability of {p[bad[0]]!r}; "
                                              f"{name} needs probabilities strictly between 0 and 1 there (or strength 0 on that bit{mode['every_leg']}).")
            if mode["route"] and self._no_decimation_kernel():
                if self._decimation_lane_node:
                    raise NotImplementedError(f"{key}: neither lane = edge kernel family nor the lane = node kernel takes this code (rows of at most 16 entries and "
                                              "columns of at most 8, a syndrome's state within LDS); a per-pass route is not built.")
                raise NotImplementedError(f"{key}: neither lane = edge kernel family takes this code (rows of at most 4 entries and columns of at most 2 "
                                          "within 1024 slots, or rows of at most 8 and columns of at most 4 within the kernels' ladder; every column used); "
                                          "the lane = node route for larger codes and a per-pass route are not built yet.")

    # ---- device engine --------------------------------------------------------------------------
    def _get_engine(self):
        """Create / refresh the HIP handle lazily so that construction and validation need no GPU."""
        from ldpc_amd.engine import HipBpEngine, HipBpMultiEngine
        if self._engine is None:
            if self._device_ids is not None:
                self._engine = HipBpMultiEngine(self._h.indptr, self._h.indices, self.n, self._channel_probs,
                                                self._max_iter, self._bp_method, self._ms_scaling_factor, self._device_ids)
            else:
                self._engine = HipBpEngine(self._h.indptr, self._h.indices, self.n, self._channel_probs,
                                           self._max_iter, self._bp_method, self._ms_scaling_factor,
                                           device=self._device)
            self._channel_dirty = False
            self._engine_key = (self._max_iter, self._bp_method, self._ms_scaling_factor)
        if self._channel_dirty:  # the reference re-reads channel_probabilities on every decode (bp.hpp:149-151)
            self._engine.set_channel(self._channel_probs)
            self._channel_dirty = False
        key = (self._max_iter, self._bp_method, self._ms_scaling_factor)
        if key != self._engine_key:
            self._engine.set_params(*key)
            self._engine_key = key
        sched = (self._schedule, None if self._schedule == PARALLEL else tuple(int(v) for v in self._serial_schedule_order))
        if sched != getattr(self, "_engine_sched", (PARALLEL, None)):
            if self._schedule == PARALLEL:
                self._engine.set_schedule("parallel")
            else:  # (re)sets the object's serial_schedule_order, the state serial_relative / the random schedule work on
                self._engine.set_schedule({SERIAL: "serial", SERIAL_RELATIVE: "serial_relative"}[self._schedule],
                                          np.asarray(self._serial_schedule_order, np.int32))
            self._engine_sched = sched
        if self._message_dtype != self._engine_dtype:
            self._engine.set_message_dtype(self._message_dtype)
            self._engine_dtype = self._message_dtype
        # (read only by float32 decodes -- which several GPUs refuse: _require_modes -- so it is pushed to a single engine only)
        if self._device_ids is None and self._float32_lane_node != self._engine_float32_lane_node:
            self._engine.set_f32_lane_node(self._float32_lane_node)
            self._engine_float32_lane_node = self._float32_lane_node
        # memory min-sum, Relay-BP, guided decimation: the handle holds at most one -- first off what it holds that is no longer wanted, then on what is
        variants = (("_memory", "_engine_memory", "set_memory"), ("_relay", "_engine_relay", "set_relay"), ("_decimation", "_engine_decimation", "set_decimation"))
        stale = [v for v in variants if not _same_setting(getattr(self, v[0]), getattr(self, v[1]))]
        for wanted, held, setter in stale:
            if getattr(self, wanted) is None:
                getattr(self._engine, setter)(None)
                setattr(self, held, None)
        for wanted, held, setter in stale:
            value = getattr(self, wanted)
            if value is not None:
                getattr(self._engine, setter)(*(value if isinstance(value, tuple) else (value,)))
                setattr(self, held, value if isinstance(value, tuple) else value.copy())
        # (read only while the decimation is on -- which is never the case on several GPUs: _require_modes -- so only then is it pushed)
        if self._decimation is not None and self._decimation_lane_node != self._engine_decimation_lane_node:
            self._engine.set_decimation_lane_node(self._decimation_lane_node)
            self._engine_decimation_lane_node = self._decimation_lane_node
        rnd = (bool(self._random_serial_schedule), self._random_schedule_seed, self._seed_epoch)
        if rnd != getattr(self, "_engine_random", (False, 0, 0)):
            self._engine.set_random_serial(rnd[0], rnd[1])  # re-seeds, as bpd.set_random_schedule_seed does (pyx:553-554)
            self._engine_random = rnd
        return self._engine

    def _get_cy(self):
        """The Cython-bound C++ host object (None if the extension is not built or the ctypes backend was requested)."""
        if self._backend == "ctypes" or self._device_ids is not None:
            return None
        if self._cy is None:
            try:
                import torch  # noqa: F401  (load torch's HIP runtime first, see ldpc_amd/_lib.py)
                from ldpc_amd.bp_decoder import _bp_core
            except ImportError:
                if self._backend == "cython":
                    raise
                self._backend = "ctypes"
                return None
            self._cy = _bp_core.CyBpCore(self._h.indptr, self._h.indices, self.n, self._channel_probs, self._max_iter,
                                         self._bp_method, self._ms_scaling_factor, self._device)
            self._cy_channel = self._channel_probs.copy()
        # push the mutable members, as the reference's setters write bpd.* directly (pyx:180-223, 342-394)
        if not np.array_equal(self._cy_channel, self._channel_probs):
            self._cy.channel_probabilities = self._channel_probs
            self._cy_channel = self._channel_probs.copy()
        self._cy.maximum_iterations = self._max_iter
        self._cy.bp_method = self._bp_method
        self._cy.ms_scaling_factor = self._ms_scaling_factor
        self._cy.message_dtype = 1 if self._message_dtype == "float32" else 0
        self._cy.float32_lane_node = self._float32_lane_node
        return self._cy

    def _decode_numpy(self, synd2d, want_llr=True, osd0=False, llr_out=None, channel_probs=None):
        """(B, m) uint8 NumPy -> (decoding, llr, iterations, converge) through the active backend.  ``llr_out``: a (B, n) float64
        C-contiguous array to receive the log-ratios instead of a new one.  ``channel_probs``: checked (B, n) row priors or None."""
        # (the schedule setters and the memory strengths live on the ctypes engine)
        self._last_batch = max(1, len(synd2d))  # (float32_route)
        cy = self._get_cy() if self._schedule == PARALLEL and self._memory is None and self._relay is None and self._decimation is None else None
        if cy is None:
            self._relay_batch = max(1, len(synd2d))  # (relay_route)
        if cy is not None and channel_probs is not None:
            return cy.decode_batch(np.ascontiguousarray(synd2d, np.uint8), want_llr, osd0, llr_out, channel_probs)
        if cy is not None:
            return cy.decode_batch(np.ascontiguousarray(synd2d, np.uint8), want_llr, osd0, llr_out)
        if channel_probs is not None:
            return self._get_engine().decode_batch(synd2d, want_llr=want_llr, osd0=osd0, llr_out=llr_out, channel_probs=channel_probs)
        return self._get_engine().decode_batch(synd2d, want_llr=want_llr, osd0=osd0, llr_out=llr_out)

    def _row_probs(self, input_vectors, channel_probs, as_syndrome=True):
        """``channel_probs`` of ``decode_batch``: what cannot be done is refused with its reason, then the array is checked
        (``HipBpEngine._row_probs``) -- without a GPU: shape, dtype, range and place need none."""
        from ldpc_amd.engine import HipBpEngine
        self._require_modes("channel_probs: per-row channel probabilities are decoded {only}")
        if self._schedule != PARALLEL:
            raise NotImplementedError(f"channel_probs with schedule='{self.schedule}': the serial schedules decode with the decoder's own "
                                      "channel probabilities only; per-row probabilities need schedule='parallel'.")
        if not as_syndrome:
            raise NotImplementedError("channel_probs with received vectors (input_vector_type='received_vector'): per-row probabilities are "
                                      "available for syndrome decoding only.")
        if self._device_ids is not None:
            raise NotImplementedError("channel_probs with device_ids=[...]: the rows of channel_probs are not sharded over several GPUs; "
                                      "decode on one GPU.")
        shim = HipBpEngine.__new__(HipBpEngine)  # (the check reads n only; no handle is made -- __del__ finds none)
        shim.n = self.n
        return HipBpEngine._row_probs(shim, input_vectors, channel_probs)

    # Whether ``decode_batch`` may overwrite the log-ratio array it handed out last time (same shape).  Off by default: ownership is never
    # inferred (reference counts are an interpreter detail -- CPython 3.14 borrows stack references, other interpreters have none).  A
    # caller who is done with ``log_prob_ratios_batch`` when the next call starts sets this (or passes ``reuse_log_prob_ratios=True`` /
    # its own array as ``log_prob_ratios_out``): at 65 536 x 10 000 the array is 5.2 GB, and a new one per call costs 1.3 million
    # first-touch faults going in and a 0.27 s ``munmap`` of the old one.
    recycle_log_prob_ratios = False

    def _llr_destination(self, rows: int, out=None, reuse=None):
        """Where a batch's log-ratios go: the caller's array; else, if the caller SAID the previous batch's array may be overwritten, that
        array -- or, when there is none yet and it would be 256 MiB or more, a new one on page-locked memory (``ldpc_hip_host_alloc``: the
        device-to-host copies write it directly, no staging buffer, no host-side copy); else None (the backend makes an ordinary array)."""
        if out is not None:
            if not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == (rows, self.n) and out.flags.c_contiguous and out.flags.writeable):
                raise ValueError(f"log_prob_ratios_out must be a writeable C-contiguous float64 array of shape ({rows}, {self.n}).")
            return out
        if self.recycle_log_prob_ratios if reuse is None else reuse:
            old = getattr(self, "log_prob_ratios_batch", None)
            if isinstance(old, np.ndarray) and old.dtype == np.float64 and old.shape == (rows, self.n) and old.flags.c_contiguous and old.flags.writeable:
                return old
            # nothing to reuse yet: the caller has said the array will be written again and again -- that is when page-locked memory pays
            # (a caller on the default path gets an ordinary array: a pinned block used once as an ordinary array is a waste of a limited resource)
            nbytes = rows * self.n * 8
            if nbytes >= (256 << 20):
                from .._lib import PinnedBlock
                blk = PinnedBlock.try_new(nbytes)
                if blk is not None:
                    return blk.array((rows, self.n), np.float64)
        return None

    def _require_parallel(self):
        """Every schedule of the reference runs on the device: 'parallel' (bp.hpp:192-325), 'serial' (bp.hpp:451-545) with a
        fixed order, and the two that keep state in the decoder object -- 'serial_relative' and random_serial_schedule
        (bp.hpp:467-483; include/ldpc_hip.h: ldpc_hip_bp_set_schedule).  For those, ``decode`` calls follow one another as on
        a reference object (the order / generator carry over); the rows of a ``decode_batch`` each start from the state at the
        time of the call."""
        return None

    def _schedule_keeps_state(self) -> bool:
        return self._schedule != PARALLEL and (self._schedule == SERIAL_RELATIVE or bool(self._random_serial_schedule))

    def _pull_schedule_state(self):
        """After a decode with a schedule that rearranges ``serial_schedule_order`` (bp.hpp:467-483): read it back, as the
        reference's property shows the decoder object's rearranged member."""
        if self._schedule_keeps_state() and self._engine is not None and hasattr(self._engine, "schedule_order"):
            self._serial_schedule_order = self._engine.schedule_order().astype(np.int64)
            self._engine_sched = (self._schedule, tuple(int(v) for v in self._serial_schedule_order))


def _same_setting(a, b) -> bool:
    """A variant's setting on the decoder and the one its handle holds: the same object, or equal arrays (memory strengths)."""
    return a is b or (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and np.array_equal(a, b))


def _zero_rows(vec: np.ndarray) -> np.ndarray:
    """(B,) bool: rows of a C-contiguous (B, w) uint8 array that are all zero (eight bytes at a time where the row length allows)."""
    if vec.shape[1] and vec.shape[1] % 8 == 0:
        return ~vec.view(np.uint64).any(axis=1)
    return ~vec.any(axis=1)


class BpDecoder(BpDecoderBase):
    """Belief-propagation decoder for binary linear codes (drop-in for ``ldpc.BpDecoder``, pyx:581-709)."""

    def __init__(self, pcm, *, error_rate=_UNSET, error_channel=_UNSET, max_iter=_UNSET, bp_method=_UNSET,
                 ms_scaling_factor=_UNSET, schedule=_UNSET, omp_thread_count=_UNSET, random_schedule_seed=_UNSET,
                 serial_schedule_order=_UNSET, input_vector_type: str = "auto", random_serial_schedule=_UNSET,
                 **kwargs):
        """Keywords as in the reference (pyx:620-623): ``error_rate: float``, ``error_channel``,
        ``max_iter: int = 0`` (0 -> n), ``bp_method: str`` ('product_sum' | 'minimum_sum' and aliases),
        ``ms_scaling_factor = 1.0``, ``schedule = 'parallel'``, ``omp_thread_count = 1``,
        ``random_schedule_seed = 0``, ``serial_schedule_order = None``, ``input_vector_type = 'auto'``,
        ``random_serial_schedule = False``, ``channel_probs`` (ldpc_v1 alias of ``error_channel``).

        Only keywords the caller actually passes reach the base initialiser -- in the reference Cython
        forwards the call's own kwargs to ``BpDecoderBase.__cinit__``, whose ``kwargs.get`` defaults
        (pyx:90-100) therefore win over the signature's: an omitted ``bp_method`` means product_sum
        (pinned by python_test/test_bp_decoder.py:121-136).
        """
        _check_pcm_type(pcm)
        given = dict(error_rate=error_rate, error_channel=error_channel, max_iter=max_iter, bp_method=bp_method,
                     ms_scaling_factor=ms_scaling_factor, schedule=schedule, omp_thread_count=omp_thread_count,
                     random_schedule_seed=random_schedule_seed, serial_schedule_order=serial_schedule_order,
                     random_serial_schedule=random_serial_schedule)
        passed = dict(kwargs)
        passed.update({k: v for k, v in given.items() if v is not _UNSET})
        # order of events in the reference: the base class's __cinit__ runs first, with every keyword (its setters raise
        # their own errors); then this class's signature is type-checked; then its body (pyx:620-629)
        super().__init__(pcm, **passed)
        _typed("error_rate", passed.get("error_rate"), float)
        _typed("max_iter", passed.get("max_iter", 0), int)
        _typed("bp_method", passed.get("bp_method", "minimum_sum"), str)
        _typed("schedule", passed.get("schedule", "parallel"), str)
        _typed("omp_thread_count", passed.get("omp_thread_count", 1), int)
        _typed("random_schedule_seed", passed.get("random_schedule_seed", 0), int)
        _typed("serial_schedule_order", passed.get("serial_schedule_order"), list)
        _typed("input_vector_type", input_vector_type, str, optional=False)
        for key in kwargs.keys():  # pyx:625-627
            if key not in ["channel_probs", "_device", "_backend", "device_ids"]:
                raise ValueError(f"Unknown parameter '{key}' passed to the BpDecoder constructor.")
        self.input_vector_type = input_vector_type  # pyx:629

    # ---- single input, reference signature (pyx:642-695) ----------------------------------------
    def decode(self, input_vector: np.ndarray) -> np.ndarray:
        _typed("input_vector", input_vector, np.ndarray, optional=False)
        ln = len(input_vector)
        if self._bp_input_type == SYNDROME and not ln == self.m:
            raise ValueError(f"The input_vector must have length {self.m} (for syndrome decoding). Not length {ln}.")
        elif self._bp_input_type == RECEIVED_VECTOR and not ln == self.n:
            raise ValueError(f"The input_vector must have length {self.n} (for received vector decoding). Not length {ln}.")
        elif self._bp_input_type == AUTO and not (ln == self.m or ln == self.n):
            raise ValueError(f"The input_vector must have length {self.m} (for syndrome decoding) or length {self.n} (for received vector decoding). Not length {ln}.")
        dtype = input_vector.dtype
        vec = np.asarray(input_vector).astype(np.uint8)  # element-wise uint8 narrowing, pyx:676-678
        if not vec.any():  # pyx:679-681 / 688-690
            self._converge = True
            return np.zeros(self.n, dtype=dtype)
        self._require_parallel()
        self._require_modes()  # (float32, memory: the one row goes through the batch kernels; the resident single-decode path is plain float64 only)
        as_syndrome = self._bp_input_type == SYNDROME or (self._bp_input_type == AUTO and ln == self.m)
        if as_syndrome:
            dec, llr, it, cv = self._decode_numpy(vec[None, :])
            out = dec[0]
        else:  # bp.hpp:162-180: decode H r, then XOR the received vector back in
            synd = self._get_engine().mulvec_batch(vec[None, :])
            dec, llr, it, cv = self._decode_numpy(synd)
            out = dec[0] ^ vec
        self._decoding = out.astype(np.uint8)
        self._log_prob_ratios = llr[0]
        self._iterations = int(it[0])
        self._converge = bool(cv[0])
        self._pull_schedule_state()
        return out.astype(dtype)

    # ---- batch (additive) -----------------------------------------------------------------------
    def decode_batch(self, input_vectors, want_log_prob_ratios: bool = True, *, log_prob_ratios_out=None, reuse_log_prob_ratios=None,
                     channel_probs=None):
        """Decode every row of a 2-D array in one launch.

        ``channel_probs``: a ``(B, n)`` float64 array in the same place as ``input_vectors`` (NumPy, or a CUDA tensor on the same GPU).  Row b is
        then decoded with ``channel_probs[b]``: ``decoding``, ``converge``, ``iter`` and ``log_prob_ratios`` of row b are what the reference
        returns for ``update_channel_probs(channel_probs[b]); decode(input_vectors[b])`` (pyx:222, 642-695) -- heralded erasures
        (p = 0.5 on the flagged bits), soft readout, drifting noise.  Probabilities 0, 1 and 0.5 are legal (priors +inf, -inf, +0.0).  Unlike that
        loop the call leaves this decoder's own ``channel_probs`` / ``error_rate`` UNCHANGED: a following plain ``decode_batch`` uses them.
        Syndromes and the parallel schedule only; ``ValueError`` for a wrong shape, a value outside [0, 1] or NaN, or arrays in different
        places; ``NotImplementedError`` for a serial schedule, received vectors and ``device_ids``.

        ``log_prob_ratios_out`` (NumPy inputs): a ``(B, n)`` float64 C-contiguous array that receives the log-ratios;
        ``reuse_log_prob_ratios=True`` (or the attribute ``recycle_log_prob_ratios``): the array the previous call handed out as
        ``log_prob_ratios_batch`` may be overwritten by this one -- nothing is reused unless the caller says so.

        ``input_vectors``: ``(B, m)`` syndromes or ``(B, n)`` received vectors (same rule as
        ``decode``), NumPy array (any integer dtype; result has the same dtype) or a torch CUDA uint8
        tensor (results stay in HBM as torch tensors).  Row ``b`` of the result equals
        ``decode(input_vectors[b])`` of the reference, including the all-zero shortcut.  Afterwards
        ``converge_batch`` (B,) bool, ``iter_batch`` (B,) int32 (0 for shortcut rows) and
        ``log_prob_ratios_batch`` (B, n) float64 (zeros for shortcut rows) describe every row and
        the scalar properties describe the last row that actually ran BP.
        """
        from ldpc_amd.engine import _is_torch
        if input_vectors.ndim != 2:
            raise ValueError("decode_batch expects a 2-D array of shape (batch, m) or (batch, n).")
        ln = int(input_vectors.shape[1])
        if self._bp_input_type == SYNDROME and not ln == self.m:
            raise ValueError(f"The input_vector must have length {self.m} (for syndrome decoding). Not length {ln}.")
        elif self._bp_input_type == RECEIVED_VECTOR and not ln == self.n:
            raise ValueError(f"The input_vector must have length {self.n} (for received vector decoding). Not length {ln}.")
        elif self._bp_input_type == AUTO and not (ln == self.m or ln == self.n):
            raise ValueError(f"The input_vector must have length {self.m} (for syndrome decoding) or length {self.n} (for received vector decoding). Not length {ln}.")
        self._require_parallel()
        self._require_modes()
        as_syndrome = self._bp_input_type == SYNDROME or (self._bp_input_type == AUTO and ln == self.m)
        if channel_probs is not None:
            channel_probs = self._row_probs(input_vectors, channel_probs, as_syndrome)
        eng = self._get_engine()
        if _is_torch(input_vectors):
            import torch
            if log_prob_ratios_out is not None or reuse_log_prob_ratios:
                raise ValueError("log_prob_ratios_out / reuse_log_prob_ratios apply to NumPy inputs only: with device tensors the log-ratios "
                                 "are returned as a device tensor (log_prob_ratios_batch).")
            vec = input_vectors
            synd = vec if as_syndrome else eng.mulvec_batch(vec)
            dec, llr, it, cv = (eng.decode_batch(synd, want_llr=want_log_prob_ratios) if channel_probs is None else
                                eng.decode_batch(synd, want_llr=want_log_prob_ratios, channel_probs=channel_probs))
            if not as_syndrome:
                dec ^= vec
            zero = vec.any(dim=1).logical_not()  # all-zero shortcut rows (pyx:679-681); uint8.any() is uint8
            if bool(zero.any()):
                dec[zero] = 0
                cv[zero] = 1
                it[zero] = 0
                if llr is not None:
                    llr[zero] = 0
            self.converge_batch, self.iter_batch, self.log_prob_ratios_batch = cv.bool(), it, llr
            self._pull_schedule_state()
            return dec
        dtype = input_vectors.dtype
        vec = np.ascontiguousarray(np.asarray(input_vectors).astype(np.uint8, copy=False))
        synd = vec if as_syndrome else eng.mulvec_batch(vec)
        # which rows take the all-zero shortcut (pyx:679-681): a scan of the whole input -- on a helper thread for large batches, while
        # the device decodes (the C call releases the GIL)
        zero_box = []
        scan = None
        if vec.size >= (1 << 24):
            import threading
            scan = threading.Thread(target=lambda: zero_box.append(_zero_rows(vec)))
            scan.start()
        try:
            dec, llr, it, cv = self._decode_numpy(synd, want_llr=want_log_prob_ratios,
                                                  llr_out=self._llr_destination(len(synd), log_prob_ratios_out, reuse_log_prob_ratios) if want_log_prob_ratios else None,
                                                  channel_probs=channel_probs)
        finally:
            if scan is not None:
                scan.join()
        if not as_syndrome:
            dec ^= vec
        zero = zero_box[0] if zero_box else _zero_rows(vec)
        if zero.any():
            dec[zero] = 0
            cv[zero] = True
            it[zero] = 0
            if llr is not None:
                llr[zero] = 0.0
        self.converge_batch, self.iter_batch, self.log_prob_ratios_batch = cv, it, llr
        ran = np.flatnonzero(~zero)
        if len(ran):
            last = int(ran[-1])
            self._decoding = dec[last].astype(np.uint8)
            if llr is not None:
                self._log_prob_ratios = llr[last].copy()  # (a copy, not a view: a view would pin the whole batch array)
            self._iterations = int(it[last])
        if len(vec):
            self._converge = bool(cv[-1])
        self._pull_schedule_state()
        return dec.astype(dtype, copy=False)

    @property
    def decoding(self) -> np.ndarray:
        return np.array(self._decoding).astype(int)  # pyx:698-709

    decoding = decoding.setter(_readonly("decoding", "BpDecoder"))


class SoftInfoBpDecoder(BpDecoderBase):
    """Serial minimum-sum BP with analog syndrome information (drop-in for ``ldpc.bp_decoder.SoftInfoBpDecoder``,
    pyx:712-812; algorithm ``soft_info_decode_serial``, bp.hpp:547-660).

    Keywords as in the reference (pyx:743-745): ``error_rate``, ``error_channel``, ``max_iter = 0`` (-> n),
    ``bp_method`` (ignored: always minimum_sum, pyx:752), ``ms_scaling_factor = 1.0``, ``cutoff = inf``,
    ``sigma = 2.0``.  ``decode`` takes one vector of ``m`` analog readouts; ``decode_batch`` (additive) takes ``(B, m)``.
    """

    def __init__(self, pcm, *, error_rate=_UNSET, error_channel=_UNSET, max_iter=_UNSET, bp_method=_UNSET,
                 ms_scaling_factor=_UNSET, cutoff=np.inf, sigma: float = 2.0, **kwargs):
        _check_pcm_type(pcm)
        given = dict(error_rate=error_rate, error_channel=error_channel, max_iter=max_iter, bp_method=bp_method,
                     ms_scaling_factor=ms_scaling_factor)
        passed = dict(kwargs)
        passed.update({k: v for k, v in given.items() if v is not _UNSET})
        super().__init__(pcm, **passed)
        _typed("error_rate", passed.get("error_rate"), float)  # the signature of pyx:743-745, checked after the base class ran
        _typed("error_channel", passed.get("error_channel"), list)
        _typed("max_iter", passed.get("max_iter", 0), int)
        _typed("bp_method", passed.get("bp_method", "minimum_sum"), str)
        _typed("ms_scaling_factor", passed.get("ms_scaling_factor", 1.0), float)
        _typed("cutoff", cutoff, float)
        sigma = _c_double(sigma)
        self.cutoff = cutoff
        if not isinstance(sigma, float) or sigma <= 0:  # pyx:748-749
            raise ValueError("The sigma value must be a float greater than 0.")
        self.sigma = sigma
        self.schedule = "serial"
        self.bp_method = "minimum_sum"
        self.input_vector_type = "syndrome"
        self._soft_syndrome = np.zeros(self.m, np.float64)
        self.soft_syndrome_batch = None

    def _soft_decode(self, soft2d):
        """With random_serial_schedule the routine rearranges the order the object carries at the top of every iteration it runs
        (bp.hpp:573-577: ``shuffle(order, std::default_random_engine(random_schedule_seed))``, a new engine each time); the engine
        does the same draws, every row of a batch from the order at the time of the call, and leaves its last row's order."""
        self._require_modes("soft-syndrome decoding: it is a serial schedule (bp.hpp:547-660)")
        out = self._get_engine().soft_info_decode_batch(soft2d, self.cutoff, self.sigma)
        self._pull_schedule_state()
        return out

    def decode(self, soft_info_syndrome: np.ndarray) -> np.ndarray:
        """One analog syndrome (pyx:761-785); returns the decoding as uint8."""
        soft = np.asarray([soft_info_syndrome[i] for i in range(self.m)], dtype=np.float64)  # pyx:776-779
        dec, llr, it, cv, so = self._soft_decode(soft[None, :])
        self._decoding = dec[0].copy()
        self._log_prob_ratios = llr[0]
        self._iterations = int(it[0])
        self._converge = bool(cv[0])
        self._soft_syndrome = so[0]
        return dec[0].astype(np.uint8)

    def decode_batch(self, soft_info_syndromes, channel_probs=None):
        """``(B, m)`` analog syndromes in one launch; row b equals ``decode(soft_info_syndromes[b])``.  Afterwards
        ``converge_batch``, ``iter_batch``, ``log_prob_ratios_batch`` and ``soft_syndrome_batch`` describe every row."""
        if channel_probs is not None:
            raise NotImplementedError("channel_probs with SoftInfoBpDecoder: soft-syndrome decoding is a serial schedule (bp.hpp:547-660) and "
                                      "decodes with the decoder's own channel probabilities only.")
        if soft_info_syndromes.ndim != 2 or soft_info_syndromes.shape[1] != self.m:
            raise ValueError(f"The soft syndromes must have shape (batch, {self.m}).")
        from ldpc_amd.engine import _is_torch
        soft = soft_info_syndromes if _is_torch(soft_info_syndromes) else np.ascontiguousarray(soft_info_syndromes, np.float64)
        dec, llr, it, cv, so = self._soft_decode(soft)
        self.converge_batch, self.iter_batch, self.log_prob_ratios_batch, self.soft_syndrome_batch = cv, it, llr, so
        return dec

    @property
    def soft_syndrome(self) -> np.ndarray:
        return np.array(self._soft_syndrome, dtype=np.float64)

    @property
    def decoding(self) -> np.ndarray:
        return np.array(self._decoding).astype(int)
