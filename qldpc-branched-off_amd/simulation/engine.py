"""``run_simulation`` with the reference's signature and result keys (src/simulation/engine.py:193-488), batched on GPUs.

The reference spawns a process pool and runs one trial per task (engine.py:433-457); here all trials of a batch run
concurrently on the device (qldpc_circuit_plan_*), the tally stays on the device, and with several ranks
(torch.distributed) each rank takes a contiguous trial range followed by ONE all-reduce of the tally.

Differences that are deliberate and documented:
  * randomness comes from Philox streams keyed by (base_seed, global trial index), not from legacy ``np.random``; results
    are reproducible and independent of the number of GPUs, and statistically equivalent to the reference;
  * the alpha / beta estimators (``alpha_mode='alvarado*'``, ``scopt=True``) draw from ``default_rng(base_seed)`` instead of an
    unseeded Generator, so all ranks agree on the factors; their trial loops run on the GPU (qldpc_msgstats_*);
  * ``osd_order > 0``: the reference returns the OSD-0 solution whenever it reproduces the syndrome (osd.py:27-29), which it always
    does for syndromes the circuit itself generates -- those trials stay on the fused device pipeline.  A batch in which some trial
    ends unsatisfied (possible with foreign ``precomputed_matrices``) is decoded again through the batched OSD-w sweep
    (qldpc_osdw_batch, osd.py:31-75) for the shots BP failed on, so the result is the reference's for every input;
  * ``num_workers`` keeps the reference's meaning -- how many workers ONE call spreads its trials over (engine.py:204,433-435) -- with a worker
    being a GPU instead of a pool process: the call creates one plan per worker (its own graphs, buffers and stream on its device), hands every
    worker a contiguous trial range per round from a host thread each (the C ABI releases the GIL), and sums the tallies on the host.
    ``num_workers=None`` = every visible GPU (1 on a one-GPU box), a larger request is capped at the visible count; ``devices=[...]`` (extension)
    names the GPU of each worker explicitly and may repeat one ([0, 0] = two plans sharing a card).  Results do not depend on it;
  * one process per GPU also works: under a ``torch.distributed`` launch a rank drives ``device`` = LOCAL_RANK alone (``num_workers`` then counts
    the plans of that rank, default 1) and one all-reduce of the tally follows; with the RCCL backend it runs on device tensors;
  * ``target_logical_errors`` stops at the exact trial the reference would (in-order prefix cut over per-trial verdicts).

The extensions below choose what a worker's plan decodes with, on the plan's two axes.  The path: at most one of
``decoder="relay_bp"``, ``window=...``, ``schedule="layered"``, ``decimation=...``, ``precision="f32"``, ``correlated=...``, ``erasure={..., "aware": True}`` and ``soft={..., "aware": True}`` leaves flooding min-sum, and none of them
goes with the reference's OSD-w pass (``osd_order > 0`` with ``decoder="bp_osd"``).  The OSD stage: ``decoder="bp_osd_cs"`` puts OSD-CS in the place
of OSD-0 and ``decoder="bp_lsd"`` puts BP+LSD there; each goes with every path but Relay-BP (which has no OSD stage) and windows.  Anything else raises ValueError before any device call.

``decoder="relay_bp"`` (an extension; ``"bp_osd"`` is the default) decodes both sectors with Relay-BP (``decoding/relay.py``) instead of
min-sum + OSD-0, with ``relay_params`` over ``_lib.RELAY_DEFAULTS``.  Relay-BP uses its own constant alpha, so the alpha / beta estimators do not run,
and the arguments that only mean something for BP+OSD (``alpha_mode``, ``alvarado_alpha``, ``scopt=True``, ``osd_order > 0``) raise ValueError.
The result then also holds ``decoder``, ``relay_params`` and ``mean_legs_z`` / ``mean_legs_x`` (legs per trial).

``decoder="bp_osd_cs"`` (an extension) runs OSD-CS (``decoding/osd_cs.py``: OSD-0 followed by a combination sweep, Roffe et al. 2020) in the
plan's OSD stage, with the plan's priors as the weights.  Here ``osd_order`` is the sweep's order lambda (0..64; pairs among the lambda least
reliable non-pivot columns), not the reference's OSD-w order.  The alpha / SCOPT estimators run as for ``"bp_osd"``; ``relay_params`` raises
ValueError.  OSD-CS returns OSD-0's answer wherever the syndrome is not reproducible, so no OSD-w pass follows.  The result also holds
``decoder`` and ``osd_order``.

``decoder="bp_lsd"`` (an extension) runs BP+LSD (``decoding/lsd.py``: cluster-local post-processing, Hillmann et al. 2024) in the plan's OSD stage,
with ``lsd={"bits_per_step": 1, "max_rows": 512}`` (either key may be left out).  Its rules are those of ``"bp_osd_cs"``, and ``osd_order`` must be 0.
A trial whose clusters would pass ``max_rows`` rows, or whose residual no column reaches, gets OSD-0's answer.  The result also holds ``decoder``,
``lsd`` (the parameters used) and ``lsd_counts`` (int64[2, 3]: trials per sector that ended solved in clusters / capped / without candidates).

``window=(W, C)`` (an extension; ``decoder="bp_osd"`` with ``osd_order=0`` only) decodes both sectors with the
sliding-window decoder (``decoding/window.py``): W syndrome cycles at a time, the first C of them committed, min-sum + OSD-0 per window.  The
window graphs do not grow with ``num_cycles``.  The result also holds ``window``.

``schedule="layered"`` (an extension; ``"flooding"`` is the default and today's behaviour) runs the BP stage of both sectors with the layered
schedule (``decoding/layered.py``); only that stage changes, OSD-0 (``decoder="bp_osd"``) or OSD-CS (``decoder="bp_osd_cs"``) follows as before.
``layers=(row_layer_z, row_layer_x)`` names the layers (either may be None = the greedy colouring).  The alpha / SCOPT estimators measure flooding
messages, so anything that would run one raises ValueError (``alpha_mode="alvarado"`` without ``alvarado_alpha``, ``"alvarado-autoregressive"``,
``scopt=True``).  The result also holds ``schedule`` and ``layers_z`` / ``layers_x`` (layer counts).

``decimation={...}`` (an extension; None is today's behaviour) runs the BP stage of both sectors as BP with guided decimation
(``decoding/decimation.py``); the dict holds any of ``alpha, t_round, max_rounds, per_round, fix_llr`` (``_lib.DECIM_DEFAULTS`` for the rest).  Only
that stage changes: OSD-0 (``decoder="bp_osd"``, ``osd_order=0``) or OSD-CS (``decoder="bp_osd_cs"``) follows on the unconverged trials as before.  Its
alpha is the constant of the dict and ``maxIter`` is not used by it, so every argument that selects or estimates another alpha raises ValueError
(``alpha_mode``, ``alvarado_alpha``, ``use_dynamic_alpha=False``, ``scopt=True``).  The result also holds ``decimation`` (the parameters used) and
``mean_rounds_z`` / ``mean_rounds_x``.

``precision="f32"`` (an extension; ``"f64"`` is the default and today's behaviour) runs the BP stage of both sectors in single precision
(``decoding/single.py``): the plan's priors, alpha table, ``maxIter`` and clip rounded to f32, every operation one f32 operation.  Only that stage
changes; OSD-0 (``decoder="bp_osd"``, ``osd_order=0``) or OSD-CS (``decoder="bp_osd_cs"``) follows as before.  The alpha / SCOPT estimators stay
f64: the alpha they return is rounded to f32 like any other.  Results differ from ``"f64"`` in some trials (rounding, amplified by the iteration);
compare logical error rates, not trials.  The result holds ``precision``.

``correlated={"alpha": 1.0, "mode": "raise"}`` (an extension; None is today's behaviour; either key, and ``floor``, may be left out) decodes the two
sectors in two passes (``simulation/correlated.py``): sector Z as constant-alpha min-sum, then sector X with a per-shot prior in which every column that
shares a fault with a column of sector Z's correction is raised to its conditional probability.  The links come from ``links_from_circuit`` at
``error_rate``.  OSD-0, OSD-CS (which still scores with the shared prior) or LSD follows on the unconverged trials as before.  Its alpha is the constant of
the dict, so every argument that selects or estimates another alpha raises ValueError, as for ``decimation``.  The result also holds ``correlated`` and
``correlated_links``.

``erasure={"rates": ..., "aware": True, "alpha": 1.0}`` (an extension; None is today's behaviour; ``aware`` defaults to True and ``alpha`` to 1.0) adds
heralded-erasure noise to the sampler (``simulation/erasure.py``, ``CircuitPlan.use_erasure_noise``): ``rates`` is a number (every location class) or a
dict keyed by the gate names CNOT, PrepX, PrepZ, MeasX, MeasZ, IDLE.  With ``aware=True`` both sectors are decoded with a per-shot prior built from the
heralds (``CircuitPlan.use_erasure_aware``, the tables of ``erasure_tables_from_circuit``): a decode path, so it goes with none of the others, its alpha
is the constant of the dict as for ``correlated``, and OSD-0, OSD-CS (which still scores with the shared prior) or LSD follows as before.  With
``aware=False`` only the sampler changes -- the sampler axis -- and every path and decoder goes with it: the decoder does not see the heralds.  The result
also holds ``erasure`` (rates as f64[7] by op code, aware, alpha).  Circuit plans only: ``run_weight_strata`` and ``run_dem_simulation`` raise ValueError.

``soft={"sigma": 0.4, "levels": 8, "aware": True, "alpha": 1.0}`` (an extension; None is today's behaviour; ``levels`` defaults to 8, ``aware`` to True
and ``alpha`` to 1.0; ``{"readout": SoftReadout(...)}`` gives the channel itself) adds soft-readout noise to the sampler (``simulation/soft.py``,
``CircuitPlan.use_soft_readout``): every measurement gets a readout flip and a confidence level.  With ``aware=True`` both sectors are decoded with a
per-shot prior built from the levels (``CircuitPlan.use_soft_aware``, the tables of ``soft_tables_from_circuit``): a decode path under the rules of
``erasure``'s.  With ``aware=False`` only the sampler changes and every path and decoder goes with it.  With ``matched_priors=True`` (the default) the
plan's priors are ``marginal_priors`` -- the readout's marginal flip rate folded into the measured columns, what a decoder that does not read the levels
should believe -- else the plain ones.  It goes with neither ``erasure`` nor ``noise_model``.  The result also holds ``soft`` (readout, aware, alpha) and
``matched_priors``.

``noise_model=NoiseModel(...)`` (an extension; None is today's behaviour) replaces the sampler's one rate and uniform Paulis by a rate per location class
and, optionally, weighted Paulis on faulty IDLEs and CNOTs (``simulation/noise_model.py``, ``CircuitPlan.use_noise_model``): the sampler axis, so every
path and decoder goes with it.  The decoding matrices are built or loaded at ``error_rate`` as without it -- their columns do not depend on the rates
-- and with ``matched_priors=True`` (the default) both sectors' priors come from the model (``NoiseModel.prior_llrs``); ``matched_priors=False`` keeps the
uniform priors of ``error_rate``: the mismatched-decoder study.  ``correlated=...`` and ``erasure=...`` raise ValueError beside it (link masses and erasure
look-up tables under a model do not exist yet), and so does ``run_weight_strata``.  The result also holds ``noise_model`` and ``matched_priors``.
The alpha / SCOPT estimators (``alpha_mode="alvarado"`` without ``alvarado_alpha``, ``"alvarado-autoregressive"``, ``scopt=True``) are NOT taught the model:
they still draw their error patterns at the single ``error_rate`` while reading the priors the plan gets, so beside a model their factors belong to a
noise that is neither the model's nor the priors'.  Only the dynamical alpha (the default) or a given ``alvarado_alpha`` is meaningful beside a model.

``simulation/dem.py`` (``run_dem_simulation``: the same pipeline fed by a detector error model instead of a bivariate-bicycle circuit) shares the
argument rules of the extensions (``_extension_rules``), the choice of devices (``_worker_devices``) and the Worker, round loop, early stop,
all-reduce and result assembly (``_run_trials``) with ``run_simulation``; the two differ in how a worker's plan is created.
"""
import os
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

from .. import _lib, parallel
from ..decoding.alpha import estimate_alpha_alvarado, estimate_alpha_alvarado_autoregressive
from ..decoding.scopt import estimate_scopt_beta
from ..decoding.layered import check_layers, layer_count, validate_layers
from ..codes.bb_code import BBCodeCircuit
from ..noise.compiled import CompiledCircuit
from ..noise.builder import build_decoding_matrices


def prior_llrs(channel_probs):
    """engine.py:210-212: clip(nan_to_num(log((1 - p) / p)), -50, 50) (p_j > 1 -> NaN -> 0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.clip(np.nan_to_num(np.log((1 - channel_probs) / channel_probs)), -50, 50)


def _estimation_trials(requested, n_cols, error_rate):
    """engine.py:230-246: enough trials for ~2000 flipped bits, clamped to [500, 50000], unless the caller changed the default."""
    dynamic = max(500, min(50000, int(2000 / (n_cols * error_rate))))
    return requested if requested != 5000 else dynamic


def _extension_rules(osd_order, precision, decimation, schedule, layers, window, decoder, relay_params, alpha_mode, alvarado_alpha, use_dynamic_alpha, scopt,
                     maxIter, num_workers, lsd=None, correlated=None, erasure=None, soft=None):
    """The argument rules of the extensions (decoder, window, schedule, layers, decimation, precision, correlated), shared by run_simulation and
    run_dem_simulation: raises ValueError before any device call.  Returns the call on the plan's two axes -- ``path`` ("flooding", "layered",
    "decimation", "f32", "relay", "window", "correlated" or "erasure": who decodes the BP stage) and the OSD stage, ``osd_cs`` (OSD-CS instead of OSD-0) or ``lsd`` (BP+LSD instead of OSD-0: its normalised
    parameters, else None) -- with the normalised parameters of that path (``layers``, ``decimation``, ``relay_params``, ``window``, ``correlated``; None
    where the path is another), ``erasure`` (the sampler axis: rates f64[7], aware, alpha; None without erasure noise) and ``soft`` (the sampler axis
    again: readout, aware, alpha; None without soft readout; "soft" is the path where it is aware)."""
    if osd_order < 0:
        raise ValueError("osd_order must be >= 0")
    if precision not in ("f64", "f32"):
        raise ValueError(f"Unsupported precision: {precision!r} (expected 'f64' or 'f32')")
    if schedule not in ("flooding", "layered"):
        raise ValueError(f"Unsupported schedule: {schedule!r} (expected 'flooding' or 'layered')")
    if decoder not in ("bp_osd", "relay_bp", "bp_osd_cs", "bp_lsd"):
        raise ValueError(f"Unsupported decoder: {decoder!r} (expected 'bp_osd', 'relay_bp', 'bp_osd_cs' or 'bp_lsd')")
    osd_cs = decoder == "bp_osd_cs"
    if lsd is not None and decoder != "bp_lsd":
        raise ValueError("lsd is for decoder='bp_lsd'")
    if decoder == "bp_lsd":
        if osd_order != 0:
            raise ValueError(f"decoder='bp_lsd' goes with osd_order=0 (got {osd_order}): LSD takes the place of the OSD stage")
        if lsd is not None and not isinstance(lsd, dict):
            raise ValueError("lsd must be a dict with bits_per_step and / or max_rows (or None)")
        lsd = _lib.lsd_params(lsd)
    if erasure is not None:
        if not isinstance(erasure, dict) or "rates" not in erasure:
            raise ValueError("erasure must be a dict with rates and, optionally, aware and alpha (or None)")
        unknown = set(erasure) - {"rates", "aware", "alpha"}
        if unknown:
            raise ValueError(f"unknown erasure parameter(s): {sorted(unknown)}")
        if not isinstance(erasure.get("aware", True), (bool, np.bool_)):
            raise ValueError("erasure['aware'] must be True or False")
        from .erasure import erasure_rates
        erasure = {"rates": erasure_rates(erasure["rates"]), "aware": bool(erasure.get("aware", True)),
                   "alpha": _lib.shotprior_params(erasure.get("alpha", 1.0), 20.0, maxIter)[0]}
    aware = erasure is not None and erasure["aware"]
    if soft is not None:
        if not isinstance(soft, dict) or ("readout" in soft) == ("sigma" in soft):
            raise ValueError("soft must be a dict with either sigma (and, optionally, levels and edges) or readout, and, optionally, aware and alpha (or None)")
        unknown = set(soft) - ({"readout", "aware", "alpha"} if "readout" in soft else {"sigma", "levels", "edges", "aware", "alpha"})
        if unknown:
            raise ValueError(f"unknown soft parameter(s): {sorted(unknown)}")
        if not isinstance(soft.get("aware", True), (bool, np.bool_)):
            raise ValueError("soft['aware'] must be True or False")
        if erasure is not None:
            raise ValueError("soft=... does not go with erasure=... (the two samplers do not compose)")
        from .soft import SoftReadout
        readout = soft["readout"] if "readout" in soft else SoftReadout.gaussian(soft["sigma"], soft.get("levels", 8), soft.get("edges"))
        if not isinstance(readout, SoftReadout):
            raise ValueError(f"soft['readout'] must be a simulation.soft.SoftReadout, got {readout!r}")
        soft = {"readout": readout, "aware": bool(soft.get("aware", True)), "alpha": _lib.shotprior_params(soft.get("alpha", 1.0), 20.0, maxIter)[0]}
    soft_aware = soft is not None and soft["aware"]
    # the path: at most one argument leaves flooding min-sum (the plan's own rule, qldpc_circuit_plan_use_*) ...
    asked = [(path, text) for path, text, given in (("f32", "precision='f32'", precision == "f32"), ("decimation", "decimation=...", decimation is not None),
                                                     ("layered", "schedule='layered'", schedule == "layered"),
                                                     ("window", f"window={window!r}", window is not None), ("relay", "decoder='relay_bp'", decoder == "relay_bp"),
                                                     ("correlated", "correlated=...", correlated is not None),
                                                     ("erasure", "erasure={..., 'aware': True}", aware),
                                                     ("soft", "soft={..., 'aware': True}", soft_aware))
             if given]
    if len(asked) > 1:
        (_, one), (_, other) = asked[:2]
        raise ValueError(f"{one} does not go with {other}: {one} goes with none of the others of decoder='relay_bp', window=(W, C), schedule='layered', "
                         "decimation=..., precision='f32', correlated=..., erasure={..., 'aware': True} and soft={..., 'aware': True} (each decodes the BP stage its own way)")
    path, text = asked[0] if asked else ("flooding", None)
    # ... and none of them goes with the OSD-w pass, which decodes again with flooding min-sum in f64
    if path != "flooding" and decoder == "bp_osd" and osd_order > 0:
        raise ValueError(f"{text} goes with osd_order=0{'' if path == 'window' else ' or decoder=%r' % 'bp_osd_cs'} (with decoder='bp_osd', "
                         f"osd_order={osd_order} asks for the OSD-w pass, which decodes with flooding min-sum in f64)")
    if layers is not None and path != "layered":
        raise ValueError("layers is for schedule='layered'")
    if relay_params is not None and path != "relay":
        raise ValueError("relay_params is for decoder='relay_bp'")
    if osd_cs and not 0 <= int(osd_order) <= _lib.OSDCS_MAX_ORDER:
        raise ValueError(f"decoder='bp_osd_cs': osd_order is the combination-sweep order, 0..{_lib.OSDCS_MAX_ORDER} (got {osd_order})")
    # what is particular to a path (before any device call: these are argument rules)
    if path == "f32":
        _lib.check_minsum32_args(maxIter, 20.0)
    elif path == "decimation":
        if not isinstance(decimation, dict):
            raise ValueError("decimation must be a dict of guided-decimation parameters (or None)")
        bad = [name for name, given in (("alpha_mode", alpha_mode is not None), ("alvarado_alpha", alvarado_alpha is not None),
                                        ("use_dynamic_alpha=False", not use_dynamic_alpha), ("scopt", bool(scopt))) if given]
        if bad:
            raise ValueError(f"decimation=... does not use {', '.join(bad)}: its alpha is the constant decimation['alpha']")
        if "clip_llr" in decimation:
            raise ValueError("decimation: the circuit plan's clip_llr is fixed (20)")
        decimation = _lib.decim_params(decimation, with_clip=False)
    elif path == "correlated":
        if not isinstance(correlated, dict):
            raise ValueError("correlated must be a dict with alpha, mode and / or floor (or None)")
        bad = [name for name, given in (("alpha_mode", alpha_mode is not None), ("alvarado_alpha", alvarado_alpha is not None),
                                        ("use_dynamic_alpha=False", not use_dynamic_alpha), ("scopt", bool(scopt))) if given]
        if bad:
            raise ValueError(f"correlated=... does not use {', '.join(bad)}: its alpha is the constant correlated['alpha']")
        unknown = set(correlated) - {"alpha", "mode", "floor"}
        if unknown:
            raise ValueError(f"unknown correlated parameter(s): {sorted(unknown)}")
        from .correlated import check_mode
        correlated = {"alpha": _lib.shotprior_params(correlated.get("alpha", 1.0), 20.0, maxIter)[0], "mode": correlated.get("mode", "raise"),
                      "floor": correlated.get("floor")}
        check_mode(correlated["mode"], correlated["floor"])
    elif path == "erasure":
        bad = [name for name, given in (("alpha_mode", alpha_mode is not None), ("alvarado_alpha", alvarado_alpha is not None),
                                        ("use_dynamic_alpha=False", not use_dynamic_alpha), ("scopt", bool(scopt))) if given]
        if bad:
            raise ValueError(f"erasure={{..., 'aware': True}} does not use {', '.join(bad)}: its alpha is the constant erasure['alpha']")
    elif path == "soft":
        bad = [name for name, given in (("alpha_mode", alpha_mode is not None), ("alvarado_alpha", alvarado_alpha is not None),
                                        ("use_dynamic_alpha=False", not use_dynamic_alpha), ("scopt", bool(scopt))) if given]
        if bad:
            raise ValueError(f"soft={{..., 'aware': True}} does not use {', '.join(bad)}: its alpha is the constant soft['alpha']")
    elif path == "layered":
        mode = alpha_mode if alpha_mode is not None else ("dynamical" if use_dynamic_alpha else "alvarado")
        if mode == "alvarado-autoregressive" or (mode == "alvarado" and alvarado_alpha is None):
            raise ValueError(f"schedule='layered' has no alpha estimator (alpha_mode={mode!r} would run the flooding one): pass alvarado_alpha or use 'dynamical'")
        if scopt:
            raise ValueError("schedule='layered' has no SCOPT estimator (scopt=True would run the flooding one)")
        _lib.check_layered_args(maxIter, 20.0)
        if layers is None:
            layers = (None, None)
        if not isinstance(layers, (tuple, list)) or len(layers) != 2:
            raise ValueError("layers must be a pair (row_layer_z, row_layer_x); either may be None")
    elif path == "window":
        if osd_cs or lsd is not None:
            raise ValueError("window=(W, C) goes with decoder='bp_osd' and osd_order=0 only")
        if not isinstance(window, (tuple, list)) or len(window) != 2:
            raise ValueError("window must be a pair (W, C)")
        window = _lib.check_window_args(1, window[0], window[1])[1:]
    elif path == "relay":
        bad = [name for name, given in (("alpha_mode", alpha_mode is not None), ("alvarado_alpha", alvarado_alpha is not None), ("scopt", bool(scopt)),
                                        ("osd_order", osd_order > 0)) if given]
        if bad:
            raise ValueError(f"decoder='relay_bp' does not use {', '.join(bad)} (Relay-BP has its own constant alpha and no OSD stage)")
        relay_params = dict(relay_params or {})
        if "clip_llr" in relay_params:
            raise ValueError("relay_params: the circuit plan's clip_llr is fixed (20)")
        relay_params = _lib.relay_params(relay_params, with_clip=False)
    if num_workers is not None and int(num_workers) < 1:
        raise ValueError("num_workers must be >= 1")
    return SimpleNamespace(path=path, osd_cs=osd_cs, lsd=lsd, layers=layers, decimation=decimation, relay_params=relay_params, window=window, correlated=correlated,
                           links=None, erasure=erasure, erasure_tables=None, noise_model=None, matched_priors=True, soft=soft, soft_tables=None, post_select=None)


def _noise_model_rules(who, noise_model, matched_priors, correlated=None, erasure=None, soft=None):
    """The argument rules of ``noise_model=`` / ``matched_priors=``: raises ValueError before any device call."""
    if soft is not None and not isinstance(matched_priors, (bool, np.bool_)):
        raise ValueError(f"{who}: matched_priors must be True or False")
    if noise_model is None:
        return
    if soft is not None:
        raise ValueError(f"{who}: noise_model=... does not go with soft=... (the soft-readout sampler draws its ordinary faults at one rate)")
    from .noise_model import NoiseModel
    if not isinstance(noise_model, NoiseModel):
        raise ValueError(f"{who}: noise_model must be a simulation.noise_model.NoiseModel (or None), got {noise_model!r}")
    if not isinstance(matched_priors, (bool, np.bool_)):
        raise ValueError(f"{who}: matched_priors must be True or False")
    if correlated is not None:
        raise ValueError(f"{who}: noise_model=... does not go with correlated=... (the link masses are computed for one rate and uniform Paulis)")
    if erasure is not None:
        raise ValueError(f"{who}: noise_model=... does not go with erasure=... (the erasure sampler draws its ordinary faults at one rate)")


def _worker_devices(num_workers, devices, device):
    """(rank, world, devices): the rank of this process in a torch.distributed launch and which GPU each worker of THIS process drives."""
    rank, world = 0, 1
    try:
        import torch.distributed as _dist
        if _dist.is_available() and _dist.is_initialized():
            rank, world = _dist.get_rank(), _dist.get_world_size()
    except ImportError:
        _dist = None
    # which GPU each worker of THIS process drives (engine.py:204: num_workers)
    if devices is not None:
        devices = [int(d) for d in devices]
        if not devices:
            raise ValueError("devices must name at least one GPU")
    elif world > 1 or device is not None or "LOCAL_RANK" in os.environ:
        devices = [parallel.local_device(device)] * int(num_workers or 1)       # a rank of a multi-process launch: its own GPU
    else:
        visible = max(1, _lib.device_count())
        devices = list(range(min(int(num_workers), visible) if num_workers else visible))
    device = devices[0]
    if world > 1 and _dist.get_backend() == "nccl":
        import torch
        torch.cuda.set_device(device)              # RCCL collectives run on the rank's own GPU
    return rank, world, devices


def _plan_switch(rules, csr, osd_order):
    """How a fresh plan moves to the call's path (qldpc_circuit_plan_use_*; the plan itself holds the rules), shared by _run_trials and
    dem.DemDecoder: (switch, layers).  switch(plan) puts OSD-CS of `osd_order` or LSD in the OSD stage when the rules ask for it, then moves the BP stage to
    rules.path (correlated: with rules.links, the CorrelationLinks the caller built; None = no links; erasure: with rules.erasure_tables; soft: with
    rules.soft_tables), then switches erasure noise, a noise model or soft readout on where the rules ask for it (the sampler axis: last, since it goes with whatever the plan decodes with),
    then the confidence of rules.post_select (kind, edges, and the weights per sector the caller put there) on the LSD stage.  csr: (indptr, indices, n) per sector; layers: the row_layer every plan gets per sector (host code; None off the layered path)."""
    layers = None
    if rules.path == "layered":
        layers = [check_layers(c) if lay is None else validate_layers(c, lay) for c, lay in zip(csr, rules.layers)] + [None] * (2 - len(csr))
    to_path = {"flooding": lambda plan: None, "relay": lambda plan: plan.use_relay(**rules.relay_params), "window": lambda plan: plan.use_window(*rules.window),
               "layered": lambda plan: plan.use_layered(*layers), "decimation": lambda plan: plan.use_decimation(**rules.decimation),
               "f32": lambda plan: plan.use_f32(),
               "correlated": lambda plan: plan.use_correlated(rules.correlated["alpha"], rules.links, None if rules.links is None else rules.links.base),
               "erasure": lambda plan: plan.use_erasure_aware(rules.erasure["alpha"], rules.erasure_tables),
               "soft": lambda plan: plan.use_soft_aware(rules.soft["alpha"], rules.soft_tables)}[rules.path]

    def switch(plan):
        if rules.osd_cs:
            plan.use_osd_cs(int(osd_order))
        if rules.lsd is not None:
            plan.use_lsd(**rules.lsd)
        to_path(plan)
        if rules.erasure is not None:                                            # the sampler axis: goes with whatever the plan decodes with
            from .erasure import GATES                                           # (in op-code order: rates[1..6])
            plan.use_erasure_noise({g: rules.erasure["rates"][i + 1] for i, g in enumerate(GATES)})
        if rules.noise_model is not None:                                        # the sampler axis again
            plan.use_noise_model(rules.noise_model)
        if rules.soft is not None:                                               # ... and a fourth time
            plan.use_soft_readout(rules.soft["readout"])
        if rules.post_select is not None:                                        # rides on the LSD stage (simulation/postselect.py)
            plan.use_confidence(rules.post_select["kind"], rules.post_select["edges"], *rules.post_select["weights"])

    return switch, layers


def _run_trials(make_plan, graphs, llrs, masks, alphas, ks, rules, rank, world, devices, base_seed, num_trials, max_trials, target_logical_errors, maxIter,
                osd_order, alpha_mode, batch, decoder, schedule, precision, extra):
    """The trial loop and the result of run_simulation and run_dem_simulation: one Worker (plan, graphs, stream) per entry of `devices`, rounds of
    contiguous trial ranges over the workers and ranks, the in-order early stop, one all-reduce of the tally per round, and the result dict.
    make_plan(graphs, device) creates a worker's plan; graphs / llrs / masks / alphas / ks hold one entry per sector (the first worker uses `graphs`)."""
    device = devices[0]
    T = _lib.TALLY
    csr = [(g.indptr, g.indices, g.n) for g in graphs]
    if rules.post_select is not None:
        if world > 1:
            raise ValueError("post_select=... does not run under a torch.distributed world > 1 (the histogram has no multi-rank reduction)")
        rules.post_select["weights"] = [_lib.quantise_weights(prior) for prior in llrs]       # the priors the plans decode with, in units of 1 / 256
    to_path, layers = _plan_switch(rules, csr, osd_order)
    osdw_pass = osd_order > 0 and not rules.osd_cs    # (OSD-CS answers an unsatisfiable trial with OSD-0, as the fused plan does)

    class Worker:
        """One worker = the reference's pool process (engine.py:433-435) as a device plan: graphs, masks, buffers and a stream of its own on one GPU."""

        def __init__(self, dev, own_graphs=None):
            self.device = dev
            self.graphs = own_graphs or [_lib.Graph(ip, ix, n, device=dev) for ip, ix, n in csr]
            self.stream = _lib.Stream(dev)
            self.plan = make_plan(self.graphs, dev)
            to_path(self.plan)

        def osdw_batch(self, begin, count):
            """One trial range through sample -> decode -> OSD-w (order = osd_order) on the shots BP failed on -> logical comparison:
            (verdicts uint8[count] with bit0 = z_err, bit1 = x_err; tally int64[16]).  The literal per-trial pipeline of the reference
            (engine.py:68-122) with every stage batched on the device; used only for batches the fused OSD-0 plan left unsatisfied."""
            sampled = self.plan.sample(base_seed, begin, count)                          # (sparse, true) per sector
            tally = np.zeros(_lib.TALLY_SLOTS, np.int64)
            verdict = np.zeros(count, np.uint8)
            tally[T["trials"]] = count
            for sec, (g, prior, mask, alpha, k) in enumerate(zip(self.graphs, llrs, masks, alphas, ks)):
                synd, true = sampled[2 * sec], sampled[2 * sec + 1]
                det, conv, llr, iters = _lib.minsum_decode_batch(g, synd, prior, maxIter, alpha_mode, alpha)
                failed = np.flatnonzero(conv == 0)
                if failed.size:                                                          # engine.py:96-97 / 115-116
                    det[failed] = _lib.osdw_batch(g, synd[failed], llr[failed], det[failed], osd_order)
                rows = np.stack([(mask >> np.uint64(r)) & np.uint64(1) for r in range(k)]).astype(np.int64)       # k x n logical rows
                dec = (det.astype(np.int64) @ rows.T) % 2                                # engine.py:99 / 119
                err = np.any(dec != true.astype(np.int64), axis=1)                       # engine.py:100 / 120
                verdict |= (err.astype(np.uint8) << sec)
                sfx = "zx"[sec]
                tally[T[sfx + "_err"]] = int(err.sum())
                tally[T["bp_conv_" + sfx]] = int(conv.sum())
                tally[T["osd_" + sfx]] = int(failed.size)
                tally[T["iters_" + sfx]] = int((iters.astype(np.int64) + 1).sum())
                tally[T["zero_synd_" + sfx]] = int((~synd.any(axis=1)).sum())
                tally[T["unsat_" + sfx]] = int((_lib.gf2_spmv_batch(g, det) != synd).any(axis=1).sum())
            tally[T["total_err"]] = int(np.count_nonzero(verdict))
            return verdict, tally

        def run_outcomes(self, begin, count):
            """(verdicts in trial order, tally) of [begin, begin + count): the in-order early stop needs every trial's verdict (engine.py:441-464)."""
            if not count:
                return np.zeros(0, np.uint8), np.zeros(_lib.TALLY_SLOTS, np.int64)
            local = self.plan.run_outcomes(base_seed, begin, count, self.stream.ptr)
            tally = self.plan.read(self.stream.ptr, clear=True)
            if osdw_pass and (tally[T["unsat_z"]] or tally[T["unsat_x"]]):
                local, tally = self.osdw_batch(begin, count)
            return local, tally

        def run(self, begin, count):
            """tally of [begin, begin + count).  The fused plan runs OSD-0, which IS the reference's OSD-w answer whenever it reproduces the syndrome
            (osd.py:27-29) -- every syndrome a circuit can produce.  So the whole range goes through at full speed (no host round trip between batches)
            and the unsatisfied counters are looked at once; only if a trial was left unsatisfied (foreign decoding matrices) is the range redone
            batch by batch with OSD-w."""
            if count:
                self.plan.run(base_seed, begin, count, self.stream.ptr)
            tally = self.plan.read(self.stream.ptr, clear=True)
            if osdw_pass and (tally[T["unsat_z"]] or tally[T["unsat_x"]]):
                tally = np.zeros(_lib.TALLY_SLOTS, np.int64)
                for off in range(0, count, batch):
                    nb = min(batch, count - off)
                    self.plan.run(base_seed, begin + off, nb, self.stream.ptr)
                    t = self.plan.read(self.stream.ptr, clear=True)
                    if t[T["unsat_z"]] or t[T["unsat_x"]]:
                        t = self.osdw_batch(begin + off, nb)[1]
                    tally += t
            return tally

        def close(self):
            self.plan.close()
            self.stream.close()

    workers = [Worker(dev, graphs if i == 0 else None) for i, dev in enumerate(devices)]
    W = len(workers)
    pool = ThreadPoolExecutor(max_workers=W) if W > 1 else None

    def on_workers(method, begin, count):
        """`method` of every worker on its share of [begin, begin + count) (contiguous, in worker order), concurrently: one host thread per worker
        enqueues and waits -- the calls into the library release the GIL, and a thread that blocks on a full launch queue holds up its own GPU only."""
        parts = [parallel.shard_range(count, w, W) for w in range(W)]
        if pool is None:
            return [getattr(workers[0], method)(begin + parts[0][0], parts[0][1])]
        futs = [pool.submit(getattr(workers[w], method), begin + parts[w][0], parts[w][1]) for w in range(W)]
        return [f.result() for f in futs]

    if max_trials is None:
        max_trials = num_trials if num_trials is not None else 1000000
    stop_on_errors = target_logical_errors is not None and target_logical_errors > 0
    total = np.zeros(_lib.TALLY_SLOTS, np.int64)
    done = 0
    z_errs = x_errs = total_errs = 0
    lanes = world * W                                 # plans working on a round, over all ranks
    round_size = min(batch, 1024) * lanes if stop_on_errors else max_trials
    try:
        while done < max_trials:
            if stop_on_errors and done > 0:
                # size the next round from the error rate seen so far (x1.25 head-room): big batches keep the GPUs full, but every trial
                # decoded beyond the stop point is wasted work (the count itself stays exact through the prefix cut below)
                need = (target_logical_errors - total_errs) * done / max(1, total_errs) * 1.25 if total_errs else 4.0 * done
                round_size = int(min(batch * lanes, max(256 * lanes, need)))
            this = min(round_size, max_trials - done)
            begin, count = parallel.shard_range(this, rank, world)
            if stop_on_errors:
                # the reference consumes trials in index order and stops AT the trial that brings the count to the target
                # (engine.py:441-464); per-trial verdicts in shot order + a prefix cut reproduce trials_run exactly
                res = on_workers("run_outcomes", done + begin, count)
                local = np.concatenate([r[0] for r in res])
                local_tally = np.sum([r[1] for r in res], axis=0)
                verdicts = parallel.gather_in_shot_order(local, this, device=device)
                keep = parallel.cut_at_target(verdicts, total_errs, target_logical_errors)
                head = verdicts[:keep]
                z_errs += int(np.count_nonzero(head & 1))
                x_errs += int(np.count_nonzero(head & 2))
                total_errs += int(np.count_nonzero(head))
                total += parallel.allreduce_tally(local_tally, device=device)             # diagnostics only: whole rounds
                done += keep
                if total_errs >= target_logical_errors:
                    break
            else:
                local_tally = np.sum(on_workers("run", done + begin, count), axis=0)
                total += parallel.allreduce_tally(local_tally, device=device)           # engine.py:450-457
                done += this
    finally:
        if pool is not None:
            pool.shutdown(wait=True)
    extra["num_workers"] = W
    extra["devices"] = list(devices)
    plan = workers[0].plan
    try:
        ph, nbat = plan.phase_times()                                            # hipEvent spans of the plan's batches (an extension: not in the reference's result)
        extra["phase_ms_per_batch"] = {k: v / max(nbat, 1) for k, v in ph.items()}
    except _lib.QldpcError:
        pass
    if rules.lsd is not None:                                                    # flag 0 / 1 / 2 per sector over this process's plans (whole rounds, like the tally)
        extra["lsd_counts"] = np.sum([w.plan.lsd_counts(w.stream.ptr) for w in workers], axis=0)
    if rules.post_select is not None:                                            # the workers' histograms, summed on the host
        from .postselect import PostSelection
        hist = np.sum([w.plan.confidence_hist(w.stream.ptr) for w in workers], axis=0, dtype=np.uint64)
        extra["post_selection"] = PostSelection(hist, rules.post_select["edges"], rules.post_select["kind"])
    for w in workers:
        w.close()
    if stop_on_errors:
        result = {"logical_error_rate": total_errs / max(1, done), "z_logical_error_rate": z_errs / max(1, done),
                  "x_logical_error_rate": x_errs / max(1, done), "num_trials": done, "logical_errors": total_errs}     # engine.py:466-472
    else:
        result = parallel.tally_to_result(total)
    result.update(extra)
    if rules.osd_cs:
        result.update(decoder=decoder, osd_order=int(osd_order))
    if rules.lsd is not None:
        result.update(decoder=decoder, lsd=dict(rules.lsd))
    per_trial = [float(total[T[slot]]) / max(int(total[T["trials"]]), 1) for slot in ("legs_z", "legs_x")]      # Relay-BP: legs; decimation: rounds
    if rules.path == "relay":
        result.update(decoder=decoder, relay_params=dict(rules.relay_params), mean_legs_z=per_trial[0], mean_legs_x=per_trial[1])
    elif rules.path == "window":
        result.update(window=tuple(rules.window))
    elif rules.path == "layered":
        result.update(schedule=schedule, layers_z=layer_count(csr[0], layers[0]), layers_x=layer_count(csr[1], layers[1]) if len(csr) > 1 else 0)
    elif rules.path == "decimation":
        result.update(decimation=dict(rules.decimation), mean_rounds_z=per_trial[0], mean_rounds_x=per_trial[1])
    elif rules.path == "correlated":
        result.update(correlated=dict(rules.correlated), correlated_links=0 if rules.links is None else rules.links.n_links)
    if rules.erasure is not None:
        result.update(erasure=dict(rules.erasure))
    if rules.noise_model is not None:
        result.update(noise_model=rules.noise_model, matched_priors=bool(rules.matched_priors))
    if rules.soft is not None:
        result.update(soft=dict(rules.soft), matched_priors=bool(rules.matched_priors))
    result["precision"] = precision
    result["tally"] = total
    return result


def _circuit_problem(Hx, Hz, Lx, Lz, error_rate, num_cycles, precomputed_matrices, device, bb_params):
    """What a circuit plan is created from, shared by run_simulation and strata.run_weight_strata: the compiled syndrome circuit, the decoding matrices
    built at ``error_rate`` (or the precomputed ones) as graphs on ``device``, the prior LLRs and logical column masks per sector (Z, X), k, and
    ``make_plan(graphs, maxIter, alpha_z, alpha_x, alpha_mode, batch, flags)`` -> the _lib.CircuitPlan whose sampler draws at ``error_rate``."""
    cb = BBCodeCircuit(Hx, Hz, num_cycles=num_cycles, **bb_params)
    m = precomputed_matrices or build_decoding_matrices(cb, Lx, Lz, error_rate, verbose=False)          # engine.py:207-208
    compiled = CompiledCircuit(base_circuit=cb.get_full_circuit(), noiseless_suffix=cb.cycle * 2, lin_order=cb.lin_order,
                               data_qubits=cb.data_qubits, Xchecks=cb.Xchecks, Zchecks=cb.Zchecks)
    llrs_z, llrs_x = prior_llrs(np.asarray(m["channel_probsZ"], dtype=np.float64)), prior_llrs(np.asarray(m["channel_probsX"], dtype=np.float64))
    k = np.asarray(Lx).shape[0]
    graphs, masks = [], []
    for s in ("Z", "X"):
        Hdec = m[f"Hdec{s}"]
        ip, ix, shape = _lib.canonical_csr(Hdec)
        graphs.append(_lib.Graph(ip, ix, shape[1], device=device))
        if f"H{s}_logical" in m:                     # compact form: the k logical rows only (dense or (indptr, indices))
            masks.append(_lib.logical_column_masks(m[f"H{s}_logical"], shape[1]))
        else:
            flr = int(m[f"first_logical_row{s}"])
            masks.append(_lib.logical_column_masks(np.asarray(m[f"H{s}_full"])[flr:flr + k], shape[1]))    # engine.py:412-413

    def make_plan(own_graphs, maxIter, alpha_z, alpha_x, alpha_mode, batch, flags, llrs=None):
        pz, px = (llrs_z, llrs_x) if llrs is None else llrs                      # llrs: other priors for the same columns (a noise model's matched ones)
        return _lib.CircuitPlan(compiled, Lx, Lz, own_graphs[0], own_graphs[1], pz, px, masks[0], masks[1], error_rate, max_iter=maxIter,
                                alpha_z=alpha_z, alpha_x=alpha_x, alpha_mode=alpha_mode, use_osd=True, batch=batch, flags=flags)    # flags: QLDPC_FLAG_* kernel variants (extension)

    return SimpleNamespace(compiled=compiled, matrices=m, graphs=graphs, llrs=(llrs_z, llrs_x), masks=masks, k=k, make_plan=make_plan)


def run_simulation(Hx, Hz, Lx, Lz, error_rate, num_trials=1000, num_cycles=12, maxIter=50, osd_order=0, use_dynamic_alpha=True,
                   alpha_mode=None, alvarado_alpha=None, alpha_estimation_trials=5000, alpha_estimation_bins=50, precomputed_matrices=None,
                   num_workers=None, base_seed=None, use_jit=True, target_logical_errors=None, max_trials=None, scopt=False,
                   estimation_plot_dir=None, batch=16384, device=None, flags=0, devices=None, decoder="bp_osd", relay_params=None, window=None, schedule="flooding",
                   layers=None, decimation=None, precision="f64", lsd=None, correlated=None, erasure=None, noise_model=None, matched_priors=True, soft=None, post_select=None,
                   **bb_params):
    from .postselect import post_select_rules
    _noise_model_rules("run_simulation", noise_model, matched_priors, correlated, erasure, soft)
    post_select = post_select_rules("run_simulation", post_select, decoder, target_logical_errors)
    rules = _extension_rules(osd_order, precision, decimation, schedule, layers, window, decoder, relay_params, alpha_mode, alvarado_alpha,
                             use_dynamic_alpha, scopt, maxIter, num_workers, lsd=lsd, correlated=correlated, erasure=erasure, soft=soft)
    rules.post_select = post_select
    rank, world, devices = _worker_devices(num_workers, devices, device)
    device = devices[0]
    if base_seed is None:
        base_seed = int(np.random.randint(0, 2 ** 31))
    if alpha_mode is None:
        alpha_mode = "dynamical" if (use_dynamic_alpha or rules.path == "relay") else "alvarado"
    if alpha_mode not in ("dynamical", "alvarado", "alvarado-autoregressive"):
        raise ValueError(f"Unsupported alpha_mode: {alpha_mode}")
    if alpha_mode == "alvarado-autoregressive" and alvarado_alpha is not None:
        raise ValueError("alvarado_alpha must be None for alvarado-autoregressive")                       # engine.py:294-295
    if estimation_plot_dir is not None:
        os.makedirs(estimation_plot_dir, exist_ok=True)

    prob = _circuit_problem(Hx, Hz, Lx, Lz, error_rate, num_cycles, precomputed_matrices, device, bb_params)
    graphs, masks, k, (llrs_z, llrs_x) = prob.graphs, prob.masks, prob.k, prob.llrs
    if rules.path == "correlated":
        from .correlated import links_from_circuit
        rules.links = links_from_circuit(prob.compiled, Lx, Lz, prob.matrices, error_rate, rules.correlated["mode"], rules.correlated["floor"])
    if rules.path == "erasure":
        from .erasure import erasure_tables_from_circuit
        rules.erasure_tables = erasure_tables_from_circuit(prob.compiled, Lx, Lz, prob.matrices)
    own_llrs = None
    if noise_model is not None:
        rules.noise_model, rules.matched_priors = noise_model, bool(matched_priors)
        if matched_priors:                                                       # the same columns, the model's probabilities
            own_llrs = llrs_z, llrs_x = noise_model.prior_llrs(prob.compiled, Lx, Lz, prob.matrices)

    if rules.soft is not None:
        from .soft import marginal_priors, soft_tables_from_circuit
        tables = soft_tables_from_circuit(prob.compiled, Lx, Lz, prob.matrices, rules.soft["readout"])
        rules.matched_priors = bool(matched_priors)
        if rules.path == "soft":
            rules.soft_tables = tables
        if matched_priors:                                                       # the same columns, the readout's marginal flip rate on the measured ones
            own_llrs = llrs_z, llrs_x = marginal_priors(prob.matrices, tables, rules.soft["readout"])

    # Normalisation factors (engine.py:228-344).  The estimators draw their error patterns from a Generator seeded with
    # base_seed (the reference leaves it unseeded), so every rank of a multi-GPU run derives the same factors.
    extra = {}
    est_rng = np.random.default_rng(base_seed)
    rate_tag = f"{error_rate:.6g}".replace(".", "p")
    if alpha_mode == "alvarado":
        if alvarado_alpha is None:
            fits = [estimate_alpha_alvarado(g, error_rate, trials=_estimation_trials(alpha_estimation_trials, g.n, error_rate),
                                            bins=alpha_estimation_bins, rng=est_rng, plot_dir=estimation_plot_dir,
                                            plot_prefix=f"alvarado_{rate_tag}_{tag}", llrs=llr)
                    for g, llr, tag in ((graphs[0], llrs_z, "z"), (graphs[1], llrs_x, "x"))]
            (alpha_z, r2_z), (alpha_x, r2_x) = fits
        elif isinstance(alvarado_alpha, (list, tuple, np.ndarray)) and len(alvarado_alpha) == 2:
            alpha_z, alpha_x, r2_z, r2_x = float(alvarado_alpha[0]), float(alvarado_alpha[1]), None, None
        else:
            alpha_z = alpha_x = float(alvarado_alpha)
            r2_z = r2_x = None
        extra.update(alpha_r2_z=r2_z, alpha_r2_x=r2_x)                                                      # engine.py:479-481
    elif alpha_mode == "alvarado-autoregressive":
        fits = [estimate_alpha_alvarado_autoregressive(g, error_rate, maxIter=maxIter, trials=_estimation_trials(alpha_estimation_trials, g.n, error_rate),
                                                       bins=alpha_estimation_bins, rng=est_rng, plot_dir=estimation_plot_dir,
                                                       plot_prefix=f"autoregressive_{rate_tag}_{tag}", llrs=llr)
                for g, llr, tag in ((graphs[0], llrs_z, "z"), (graphs[1], llrs_x, "x"))]
        (alpha_z, r2s_z), (alpha_x, r2s_x) = fits
        extra.update(alpha_values_z=alpha_z, alpha_values_x=alpha_x, alpha_r2_values_z=r2s_z, alpha_r2_values_x=r2s_x)   # engine.py:474-478
    else:
        alpha_z = alpha_x = 1.0
    if scopt:                                                                                                # engine.py:346-387 (beta is reported, not used)
        betas = [estimate_scopt_beta(g, error_rate, trials=_estimation_trials(5000, g.n, error_rate), bins=alpha_estimation_bins, alpha=a,
                                     alpha_mode=alpha_mode, maxIter=maxIter, rng=est_rng, plot_dir=estimation_plot_dir,
                                     plot_prefix=f"scopt_{rate_tag}_{tag}", llrs=llr)
                 for g, llr, a, tag in ((graphs[0], llrs_z, alpha_z, "z"), (graphs[1], llrs_x, alpha_x, "x"))]
        extra.update(beta_z=betas[0][0], beta_x=betas[1][0], beta_r2_z=betas[0][1], beta_r2_x=betas[1][1])   # engine.py:482-486

    def make_plan(own_graphs, dev):
        return prob.make_plan(own_graphs, maxIter, alpha_z, alpha_x, alpha_mode, batch, flags, llrs=own_llrs)

    return _run_trials(make_plan, graphs, (llrs_z, llrs_x), masks, (alpha_z, alpha_x), (k, k), rules, rank, world, devices, base_seed, num_trials, max_trials,
                       target_logical_errors, maxIter, osd_order, alpha_mode, batch, decoder, schedule, precision, extra)
