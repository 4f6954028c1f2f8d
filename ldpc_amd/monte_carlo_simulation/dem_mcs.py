"""Logical error rate of a detector error model, sampled, decoded and counted on the GPU.

``MonteCarloBscSimulation`` is classical: it compares ``decoding != error``.  A circuit-noise decoder's user has a ``.dem`` file and wants
the rate at which the predicted observables differ from the true ones.  ``MonteCarloDemSimulation`` runs that loop with nothing but two
counters crossing the link per call (``HipBpEngine.simulate_b8`` / ``ldpc_hip_bp_simulate_b8``): errors are drawn with the model's own
per-mechanism probabilities, detection events and true observables are formed, the shots are decoded (BP + OSD, as
``SinterBpOsdDecoder`` decodes them) and the mismatches are counted.  The sample is the one ``noise_models.generate_dem_batch`` draws for
the same ``(seed, shot index)``; the shot index is absolute, so a run may be continued, or cut into disjoint ranges.

Several GPUs are out of scope: run one simulation per device over disjoint shot ranges (``seed`` equal, ``run_count`` / shot ranges
disjoint) and add the counts.
"""
from __future__ import annotations

import datetime
import time
from typing import Dict

import numpy as np
import scipy.sparse as sp


DECODING_PRIOR_FLOOR = 1e-9  # see MonteCarloDemSimulation._get_engine


def _model_matrices(model):
    """``(check, observables, priors)`` of whatever describes a model: DEM text / a path / a ``stim.DetectorErrorModel`` (anything
    ``ckt_noise.dem_text.load_dem`` accepts), a ``DemMatrices``, or the three matrices themselves."""
    from ldpc_amd.ckt_noise.dem_matrices import DemMatrices, detector_error_model_to_check_matrices
    if model is None:
        raise ValueError("Invalid model provided. Give DEM text, a path, a DemMatrices or (check, observables, priors).")
    if isinstance(model, DemMatrices):
        return model.check_matrix, model.observables_matrix, model.priors
    if isinstance(model, (tuple, list)):
        if len(model) != 3:
            raise ValueError("Invalid model provided. A tuple must be (check, observables, priors).")
        return model[0], model[1], model[2]
    mats = detector_error_model_to_check_matrices(model, allow_undecomposed_hyperedges=True)
    return mats.check_matrix, mats.observables_matrix, mats.priors


class MonteCarloDemSimulation:
    """``run()`` returns the ``MonteCarloBscSimulation.save()`` dictionary -- ``error_rate`` is the mean of the model's probabilities --
    plus ``bp_unconverged_count`` (rows BP left unconverged before OSD; ``None`` with a ``window_decoder``, whose windows keep theirs to
    themselves) and ``seed``.  ``run()`` continues from ``run_count``: raising ``target_run_count`` and calling it again gives the totals of
    one long run.

    ``window_decoder``: a ``BaseOverlappingWindowDecoder`` that decodes instead of BP + OSD over the whole model; per chunk the shots are
    sampled on a sampler-only handle over the whole model, unpacked on the device, put through ``predict_on_device``, and the packed
    predictions are compared on the device.  The decoder keywords (``max_iter`` .. ``message_dtype``) are then unused.

    The errors are drawn with the model's probabilities exactly; the decoder's priors are the same values clipped to
    ``[1e-9, 1 - 1e-9]``, so a mechanism at p = 0 or p = 1 keeps a finite log-ratio.  ``message_dtype="float32"`` decodes with FP32
    messages (minimum-sum only: ``bp_method="ps"`` is then refused at ``run()``, as everywhere in the library); a model beyond the lane =
    edge kernels -- most are -- then takes the per-pass kernels unless ``float32_lane_node=True`` keeps it on chip
    (``ldpc_hip_bp_set_f32_lane_node``: rows of at most 16, columns of at most 8 entries, a shot's state within LDS; same bits).  ``memory_strength``
    (``None``, a float, or one strength per mechanism in ``[-1, 1)``): memory min-sum BP, as ``BpDecoder.memory_strength``; minimum-sum with
    float64 messages only, and not together with a ``window_decoder``.  ``relay`` (a dict of ``ldpc_amd.relay_decoder.relay_schedule``
    keywords -- ``gamma0``, ``pre_iter``, ``num_sets``, ``set_max_iter``, ``gamma_dist_interval``, ``stop_nconv``, ``strengths``, ``seed``):
    Relay-BP, whose legs take the place of ``max_iter``; with ``osd_method`` OSD_0 only, and not together with ``memory_strength`` or a
    ``window_decoder``.  ``decimation`` (a dict of ``ldpc_amd.bpgd_decoder.decimation_schedule`` keywords -- ``round_iters``, ``max_rounds``,
    ``freeze_llr``): BP with guided decimation, whose rounds take the place of ``max_iter``; on models the lane = edge kernels take only
    (others are refused at ``run()``) unless ``decimation_lane_node=True`` adds the lane = node kernel for the models beyond them
    (``ldpc_hip_bp_set_decimation_lane_node``), with ``osd_method`` OSD_0 only, and not together with ``relay``, ``memory_strength`` or a
    ``window_decoder``.

    One GPU (``device``; -1: the current one).  For several, run one simulation per device over disjoint shot ranges.
    """

    def __init__(self, model, *, target_run_count, batch_size: int = 65536, seed: int = 0, max_iter: int = 0, bp_method="ms",
                 ms_scaling_factor: float = 0.625, osd_method="osd0", osd_order: int = 0, message_dtype="float64", window_decoder=None,
                 device: int = -1, memory_strength=None, relay=None, decimation=None, decimation_lane_node: bool = False,
                 float32_lane_node: bool = False) -> None:
        from ldpc_amd.bp_decoder._bp_decoder import _bp_method_code
        from ldpc_amd.noise_models.dem import check_dem_probabilities
        from ldpc_amd.sinter_decoders.sinter_bposd_decoder import _osd_code
        check, observables, priors = _model_matrices(model)
        self.check_matrix = sp.csr_matrix(check, dtype=np.uint8)
        self.check_matrix.eliminate_zeros()
        self.check_matrix.sort_indices()
        self.observables_matrix = sp.csr_matrix(observables, dtype=np.uint8)
        if self.observables_matrix.shape[1] != self.check_matrix.shape[1]:
            raise ValueError("Invalid model provided. The observables matrix must have as many columns as the check matrix.")
        self.priors = check_dem_probabilities(priors, self.check_matrix.shape[1])
        if not isinstance(target_run_count, int) or isinstance(target_run_count, bool) or target_run_count <= 0:
            raise ValueError("Invalid target run count provided.")
        self.target_run_count = target_run_count
        if not isinstance(batch_size, int) or isinstance(batch_size, bool) or batch_size <= 0:
            raise ValueError("Invalid batch size provided.")
        self.batch_size = batch_size
        if not isinstance(seed, int) or isinstance(seed, bool) or seed < 0:
            raise ValueError("Invalid seed provided. Please provide a postive integer")
        self.seed = seed
        if not isinstance(max_iter, int) or max_iter < 0:
            raise ValueError("Invalid max_iter provided.")
        self.max_iter = max_iter
        self._bp_method = _bp_method_code(bp_method)
        self.ms_scaling_factor = float(ms_scaling_factor)
        self._osd_code = _osd_code(osd_method)
        if not isinstance(osd_order, int) or osd_order < 0:
            raise ValueError("Invalid osd_order provided.")
        self.osd_order = osd_order
        if message_dtype not in ("float64", "float32"):
            raise ValueError(f"message_dtype must be 'float64' or 'float32', not {message_dtype!r}.")
        self.message_dtype = message_dtype
        if window_decoder is not None:
            if not hasattr(window_decoder, "predict_on_device"):
                raise ValueError("Invalid window_decoder provided. It must offer predict_on_device (a BaseOverlappingWindowDecoder).")
            if window_decoder.num_detectors != self.check_matrix.shape[0] or \
                    window_decoder.logical_observables_matrix.shape[0] != self.observables_matrix.shape[0]:
                raise ValueError("Invalid window_decoder provided. Its detectors and observables must be the model's.")
        self.window_decoder = window_decoder
        # memory min-sum BP (BpDecoder.memory_strength): None, a float (every mechanism) or one strength per mechanism, each finite and in [-1, 1)
        if memory_strength is not None:
            if window_decoder is not None:
                raise ValueError("memory_strength with a window_decoder: the windows decode with their own decoders, which have no memory; "
                                 "leave memory_strength at None.")
            n = self.check_matrix.shape[1]
            g = np.array(memory_strength, dtype=np.float64)
            if g.ndim == 0:
                g = np.full(n, float(g), np.float64)
            if g.shape != (n,) or not (np.isfinite(g).all() and (g >= -1.0).all() and (g < 1.0).all()):
                raise ValueError(f"Invalid memory_strength provided. It must be None, a float or {n} floats, each finite and in [-1, 1).")
            memory_strength = g
        self.memory_strength = memory_strength
        # Relay-BP (RelayBpDecoder's keywords): (strengths (legs, n), leg_iters (legs,), stop_after) or None
        if relay is not None:
            if memory_strength is not None:
                raise NotImplementedError("relay with memory_strength: the relay's legs carry their own strengths; leave memory_strength at None.")
            if window_decoder is not None:
                raise NotImplementedError("relay with a window_decoder: the windows decode with their own decoders; leave relay at None.")
            if self._osd_code in (2, 3) and self.osd_order > 0:
                raise NotImplementedError("relay with osd_method OSD_E / OSD_CS: Relay-BP is followed by OSD_0 only.")
            if not isinstance(relay, dict):
                raise ValueError("Invalid relay provided. It must be None or a dict of relay_schedule keywords.")
            from ldpc_amd.relay_decoder import relay_schedule
            relay = relay_schedule(self.check_matrix.shape[1], **relay)
        self.relay = relay
        # BP with guided decimation (BpgdDecoder's keywords): (round_iters, max_rounds, freeze_llr) or None
        if decimation is not None:
            if relay is not None:
                raise NotImplementedError("decimation with relay: the two exclude each other; leave one at None.")
            if memory_strength is not None:
                raise NotImplementedError("decimation with memory_strength: the two exclude each other; leave one at None.")
            if window_decoder is not None:
                raise NotImplementedError("decimation with a window_decoder: the windows decode with their own decoders; leave decimation at None.")
            if self._osd_code in (2, 3) and self.osd_order > 0:
                raise NotImplementedError("decimation with osd_method OSD_E / OSD_CS: guided decimation is followed by OSD_0 only.")
            if not isinstance(decimation, dict):
                raise ValueError("Invalid decimation provided. It must be None or a dict of decimation_schedule keywords.")
            from ldpc_amd.bpgd_decoder import decimation_schedule
            decimation = decimation_schedule(self.check_matrix.shape[1], **decimation)
        self.decimation = decimation
        if not isinstance(decimation_lane_node, bool):
            raise ValueError("Invalid decimation_lane_node provided. It must be a bool.")
        self.decimation_lane_node = decimation_lane_node
        if not isinstance(float32_lane_node, bool):
            raise ValueError("Invalid float32_lane_node provided. It must be a bool.")
        self.float32_lane_node = float32_lane_node
        if not isinstance(device, int) or isinstance(device, bool):
            raise ValueError("Invalid device provided.")
        self.device = device

        self.error_rate = float(self.priors.mean()) if self.priors.size else 0.0
        self.run_count = 0
        self.fail_count = 0
        self.bp_unconverged_count = None if window_decoder is not None else 0
        self.logical_error_rate = 0.0
        self.logical_error_rate_eb = 0.0
        self._engine = None

    def _get_engine(self):
        if self._engine is None:
            from ldpc_amd.engine import HipBpEngine
            h = self.check_matrix
            n = h.shape[1]
            # The sampler takes the model's probabilities as they are (p = 0 never fires, p = 1 always).  The decoder takes them clipped
            # to [DECODING_PRIOR_FLOOR, 1 - DECODING_PRIOR_FLOOR]: log((1 - p) / p) of 0 or 1 is infinite, and min-sum on infinities of
            # both signs yields NaN.  Probabilities inside the interval -- any model a circuit produces -- decode with their own value.
            decoding_priors = np.clip(self.priors, DECODING_PRIOR_FLOOR, 1.0 - DECODING_PRIOR_FLOOR)
            eng = HipBpEngine(h.indptr, h.indices, n, decoding_priors, self.max_iter if self.max_iter else max(n, 1), self._bp_method,
                              self.ms_scaling_factor, device=self.device)
            eng.set_osd(self._osd_code, 0 if self._osd_code == 1 else self.osd_order)
            eng.set_message_dtype(self.message_dtype)
            eng.set_f32_lane_node(self.float32_lane_node)
            eng.set_memory(self.memory_strength)  # (what memory min-sum cannot do -- product-sum, float32 -- is refused at run(), by the library)
            if self.relay is not None:
                eng.set_relay(*self.relay)  # (likewise)
            if self.decimation is not None:
                eng.set_decimation_lane_node(self.decimation_lane_node)
                eng.set_decimation(*self.decimation)  # (likewise -- a model no decimation kernel takes included)
            eng.set_observables(self.observables_matrix)
            eng.set_sampler(self.priors)
            self._engine = eng
        return self._engine

    # one chunk: (logical failures, rows BP left unconverged)
    def _chunk_counts(self, shot0: int, shots: int):
        eng = self._get_engine()
        if self.window_decoder is None:
            return eng.simulate_b8(self.seed, shot0, shots, chunk=shots, with_osd=True)
        import torch
        dev = torch.device("cuda", eng.device if eng.device >= 0 else torch.cuda.current_device())
        k = self.observables_matrix.shape[0]
        with torch.cuda.device(dev):
            dets, obs = eng.sample_b8(self.seed, shot0, shots, device=dev)
            predictions = self.window_decoder.predict_on_device(eng.unpack_b8(dets, eng.m))
            return eng.count_mismatch_b8(obs, eng.pack_b8(predictions.contiguous()), k), None

    def run(self) -> Dict:
        """Shots ``run_count .. target_run_count - 1`` of stream ``seed``, ``batch_size`` at a time."""
        self.start_date = datetime.datetime.fromtimestamp(time.time()).strftime("%A, %B %d, %Y %H:%M:%S")
        while self.run_count < self.target_run_count:
            shots = min(self.batch_size, self.target_run_count - self.run_count)
            fails, unconverged = self._chunk_counts(self.run_count, shots)
            self.fail_count += fails
            if unconverged is not None:
                self.bp_unconverged_count += unconverged
            self.run_count += shots
        if self.run_count:
            self.logical_error_rate = self.fail_count / self.run_count
            self.logical_error_rate_eb = float(np.sqrt(self.logical_error_rate * (1 - self.logical_error_rate) / self.run_count))
        return self.save()

    def save(self) -> Dict:
        return {"logical_error_rate": self.logical_error_rate, "logical_error_rate_eb": self.logical_error_rate_eb,
                "error_rate": self.error_rate, "run_count": self.run_count, "fail_count": self.fail_count,
                "bp_unconverged_count": self.bp_unconverged_count, "seed": self.seed}
