"""Monte-Carlo decoding of an arbitrary detector error model (DEM) on the fused device pipeline.  New here: the reference has no counterpart.

A DEM is a list of independent error MECHANISMS, each with a probability, the detectors it flips and the logical observables it flips.  It has one
or two SECTORS: decoding problems with their own detectors, Tanner graph, prior and logicals, decoded independently (like Z and X of ``run_simulation``;
sector 0 takes every ``z`` key of the result, sector 1 every ``x`` key).  One mechanism may touch both sectors -- a Y-type fault does -- so there is one
mechanism table, projected per sector.  ``run_dem_simulation`` runs sample -> decode -> OSD -> judge -> tally on a ``_lib.DemPlan``, which is a circuit
plan with another sampler: every decoder, ``use_*`` switch, the in-order early stop and ``num_workers`` come with it.

The sampler's law (``include/qldpc_hip.h``): mechanism l of trial g fires iff word ``l & 3`` of Philox4x32-10(counter (lo32 g, hi32 g, l >> 2, 3), key
(lo32 seed, hi32 seed)) is below ``floor(p_l * 2**32)``.

The mechanisms are the truth that is sampled; what the decoders see is the DECODER VIEW of a sector: a parity-check matrix over detectors, a prior per
column and a logical mask per column.  ``from_decoding_matrices`` keeps the matrices it was given as that view (the graphs and priors of today's
``run_simulation`` plan); otherwise ``decoder_view`` derives one by merging the mechanisms that look alike inside the sector.

``DemDecoder`` is the other front door of the same plan: recorded detection events in (Stim samples, hardware shots, in the model's own detector
numbering), predicted observable flips out -- events -> decode -> OSD -> predict, with the same decoders and switches and no sampler.
"""
import re
from collections import namedtuple

import numpy as np

from .. import _lib
from . import engine
from .engine import prior_llrs

DecoderView = namedtuple("DecoderView", "indptr indices shape prior logmask")      # canonical CSR over (detectors x columns), LLR prior, uint64 per column
_Sector = namedtuple("_Sector", "n_det k layer_rows det_ptr det_idx logmask")


def _columns_of(indptr, indices, n):
    """CSR (rows x n) -> (colptr int64[n + 1], rows of every column, ascending)."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    rows = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    order = np.argsort(indices, kind="stable")                 # the entries come row by row, so a stable sort leaves every column's rows ascending
    colptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(indices, minlength=n), out=colptr[1:])
    return colptr, rows[order]


class DetectorErrorModel:
    """prob f64[n_mech] and, per sector, the projection of the mechanisms onto it: ``det_ptr`` int32[n_mech + 1] / ``det_idx`` uint16 (the detectors of
    every mechanism, strictly ascending) and ``logmask`` uint64[n_mech] (bit r = observable r), with ``n_det``, ``k`` and an optional ``layer_rows`` (rows
    of one syndrome cycle, for ``window=``).  ``views``: an explicit DecoderView per sector, or None to derive it.

    ``detector_map``: per sector, an int array with the MODEL's detector number of every row of that sector -- the numbering recorded detection events
    come in (``DemDecoder``); ``n_detectors`` is the width of such a record.  None = the concatenated default: sector 0's rows are detectors
    0 .. n_det[0] - 1, sector 1's follow."""

    def __init__(self, prob, sectors, views=None, detector_map=None, n_detectors=None):
        self.prob = np.ascontiguousarray(prob, np.float64)
        if not 1 <= len(sectors) <= 2:
            raise ValueError(f"a detector error model has 1 or 2 sectors, got {len(sectors)}")
        bad = np.flatnonzero(~((self.prob >= 0) & (self.prob < 1)))
        if bad.size:
            raise ValueError(f"mechanism {int(bad[0])} has probability {self.prob[bad[0]]!r}: 0 <= p < 1 is required")
        self.sectors = []
        for s, sec in enumerate(sectors):
            n_det, k, layer_rows, det_ptr, det_idx, logmask = sec
            sec = _Sector(int(n_det), int(k), int(layer_rows or 0), np.ascontiguousarray(det_ptr, np.int32), np.ascontiguousarray(det_idx, np.uint16),
                          np.ascontiguousarray(logmask, np.uint64))
            if sec.det_ptr.size != self.prob.size + 1 or sec.logmask.size != self.prob.size:
                raise ValueError(f"sector {s}: det_ptr / logmask do not have one entry per mechanism")
            if not 0 <= sec.k <= 64:
                raise ValueError(f"sector {s}: k = {sec.k} (0..64 observables per sector)")
            if not 1 <= sec.n_det < 65536:
                raise ValueError(f"sector {s}: {sec.n_det} detectors (1..65535)")
            self.sectors.append(sec)
        self._views = list(views) if views is not None else [None] * len(self.sectors)
        if detector_map is None:
            first = np.concatenate([[0], np.cumsum([S.n_det for S in self.sectors])])
            detector_map = [first[s] + np.arange(S.n_det) for s, S in enumerate(self.sectors)]
            n_detectors = int(first[-1]) if n_detectors is None else n_detectors
        self.detector_map = [np.ascontiguousarray(x, np.int64).ravel() for x in detector_map]
        if len(self.detector_map) != len(self.sectors) or any(x.size != S.n_det for x, S in zip(self.detector_map, self.sectors)):
            raise ValueError("detector_map needs one detector number per row of every sector")
        top = max(int(x.max()) for x in self.detector_map) + 1
        self.n_detectors = top if n_detectors is None else int(n_detectors)
        if self.n_detectors < top or min(int(x.min()) for x in self.detector_map) < 0:
            raise ValueError(f"detector_map names detectors outside 0..{self.n_detectors - 1}")

    n_mech = property(lambda self: int(self.prob.size))
    n_sectors = property(lambda self: len(self.sectors))
    n_det = property(lambda self: tuple(s.n_det for s in self.sectors))
    k = property(lambda self: tuple(s.k for s in self.sectors))
    layer_rows = property(lambda self: tuple(s.layer_rows for s in self.sectors))

    def mechanism(self, l, sector=0):
        """(detectors, logmask) of mechanism l inside `sector`."""
        S = self.sectors[sector]
        return S.det_idx[S.det_ptr[l]:S.det_ptr[l + 1]].astype(np.int64), int(S.logmask[l])

    def sector(self, s):
        """The one-sector model that keeps sector s alone (every mechanism stays, so the draws of a trial do not change).  It keeps its sector's
        detector_map and the model's n_detectors: its events stay in the model's numbering."""
        return DetectorErrorModel(self.prob, [self.sectors[s]], [self._views[s]], [self.detector_map[s]], self.n_detectors)

    @classmethod
    def from_columns(cls, prob, columns, n_det, k, layer_rows=None, views=None, detector_map=None, n_detectors=None):
        """prob[l] and columns[l] = one (detectors, logmask) pair per sector, for every mechanism; detectors are XOR-ed (a repeated one cancels)."""
        nsec = len(n_det)
        layer_rows = (layer_rows,) * nsec if layer_rows is None or np.ndim(layer_rows) == 0 else tuple(layer_rows)
        sectors = []
        for s in range(nsec):
            ptr, idx, lm = [0], [], []
            for l, col in enumerate(columns):
                det, mask = col[s]
                det = np.asarray(det, np.int64).ravel()
                vals, counts = np.unique(det, return_counts=True)
                det = vals[counts % 2 == 1]
                if det.size and (det[0] < 0 or det[-1] >= n_det[s]):
                    raise ValueError(f"mechanism {l}: detector {int(det[-1] if det[-1] >= n_det[s] else det[0])} is outside sector {s} ({n_det[s]} detectors)")
                if int(mask) >> int(k[s]):
                    raise ValueError(f"mechanism {l}: logical mask {int(mask):#x} has a bit at or above k = {k[s]} (sector {s})")
                idx.append(det)
                ptr.append(ptr[-1] + det.size)
                lm.append(int(mask))
            sectors.append((n_det[s], k[s], layer_rows[s], ptr, np.concatenate(idx) if idx else np.zeros(0, np.int64), np.array(lm, np.uint64)))
        return cls(prob, sectors, views, detector_map, n_detectors)

    @classmethod
    def from_decoding_matrices(cls, m, layer_rows=None):
        """From the dict ``run_simulation(precomputed_matrices=...)`` and ``data.load_precomputed_matrices`` use (or the tag of a shipped one, e.g.
        ``"circ72"``): ``HdecZ/X``, ``channel_probsZ/X`` and ``HZ/X_logical`` (or ``H*_full`` plus ``first_logical_row*``).  The mechanisms are the columns of
        Z, then the columns of X, each touching its own sector only and firing independently with its channel probability.  A column with no detector
        and no logical bit is left out of the sampler (it is the "nothing detectable happened" column: its entry of channel_probs is a sum, not a
        probability); any other column with p outside [0, 1) raises ValueError.  The decoder view of a sector is the matrices as they are -- the same
        canonical CSR, ``prior_llrs(channel_probs)`` and logical masks ``run_simulation`` builds -- so graphs and priors are those of today's plan."""
        if isinstance(m, str):
            from ..data import load_precomputed_matrices
            m = load_precomputed_matrices(m)
        layer_rows = (layer_rows,) * 2 if layer_rows is None or np.ndim(layer_rows) == 0 else tuple(layer_rows)
        views, kept, k = [], [], []
        for s in ("Z", "X"):
            ip, ix, shape = _lib.canonical_csr(m[f"Hdec{s}"])
            n = int(shape[1])
            if f"H{s}_logical" in m:
                rows = m[f"H{s}_logical"]
                ks = (len(rows[0]) - 1) if isinstance(rows, tuple) else np.asarray(rows).shape[0]
                mask = _lib.logical_column_masks(rows, n)
            else:
                flr = int(m[f"first_logical_row{s}"])
                full = np.asarray(m[f"H{s}_full"])
                ks = int(m["k"]) if "k" in m else full.shape[0] - flr
                mask = _lib.logical_column_masks(full[flr:flr + ks], n)
            probs = np.asarray(m[f"channel_probs{s}"], dtype=np.float64)
            colptr, colrows = _columns_of(ip, ix, n)
            keep = np.flatnonzero((np.diff(colptr) > 0) | (mask != 0))
            bad = keep[~((probs[keep] >= 0) & (probs[keep] < 1))]
            if bad.size:
                raise ValueError(f"column {int(bad[0])} of Hdec{s} has channel probability {probs[bad[0]]!r}: a mechanism needs 0 <= p < 1")
            views.append(DecoderView(ip, ix, (int(shape[0]), n), prior_llrs(probs), mask))
            kept.append((keep, colptr, colrows, probs, mask))
            k.append(int(ks))
        n_mech = sum(x[0].size for x in kept)
        sectors, first = [], 0
        for s, (keep, colptr, colrows, probs, mask) in enumerate(kept):
            cnt = np.zeros(n_mech, np.int64)
            cnt[first:first + keep.size] = np.diff(colptr)[keep]
            ptr = np.concatenate([[0], np.cumsum(cnt)])
            idx = np.concatenate([colrows[colptr[j]:colptr[j + 1]] for j in keep]) if keep.size else np.zeros(0, np.int64)
            lm = np.zeros(n_mech, np.uint64)
            lm[first:first + keep.size] = mask[keep]
            sectors.append((views[s].shape[0], k[s], layer_rows[s], ptr, idx, lm))
            first += keep.size
        return cls(np.concatenate([x[3][x[0]] for x in kept]), sectors, views)

    @classmethod
    def from_text(cls, text, sector_of_detector=None):
        """Parses the flat subset of the Stim detector-error-model text format (Stim itself is not needed):

            error(p) D0 D3 L1          one mechanism; ``^`` separators count as whitespace, a repeated target cancels (XOR)
            detector(...) D5           declares an index (so does any use); coordinates are ignored
            logical_observable L2      declares an index
            # comment, blank lines

        ``repeat`` blocks and ``shift_detectors`` raise ValueError: flatten the model first (``stim.DetectorErrorModel.flattened()``).

        sector_of_detector None: one sector with every detector.  Otherwise an int array over the detectors with values 0 or 1: detector d goes to that
        sector and is renumbered inside it in ascending order.  Convention for the observables: every sector has all of them (k = the number of
        observables), and a mechanism's observable flips count in every sector in which it flips a detector; a mechanism without detectors (only L
        targets: an undetectable logical flip) counts in sector 0.  With one sector that is the usual memory experiment.

        ``detector_map[s]`` keeps the text's detector number of every row of sector s, so ``DemDecoder`` takes events in the text's numbering."""
        prob, targets, n_det, n_obs = [], [], 0, 0
        for lineno, raw in enumerate(text.splitlines(), 1):
            line = raw.split("#", 1)[0].strip()
            if not line:
                continue
            head = re.match(r"([A-Za-z_]+)\s*(\(([^)]*)\))?\s*(.*)$", line)
            name = head.group(1).lower() if head else ""
            if name in ("repeat", "shift_detectors") or line == "}":
                raise ValueError(f"line {lineno}: '{name or line}' is not supported -- flatten the detector error model first (no repeat blocks, no shift_detectors)")
            if name not in ("error", "detector", "logical_observable"):
                raise ValueError(f"line {lineno}: cannot parse {raw.strip()!r}")
            det, obs = [], 0
            for tok in head.group(4).replace("^", " ").split():
                if not re.fullmatch(r"[DL]\d+", tok):
                    raise ValueError(f"line {lineno}: bad target {tok!r}")
                i = int(tok[1:])
                if tok[0] == "D":
                    det.append(i)
                    n_det = max(n_det, i + 1)
                else:
                    if i >= 64:
                        raise ValueError(f"line {lineno}: observable {tok} -- at most 64 observables (L0..L63)")
                    obs ^= 1 << i
                    n_obs = max(n_obs, i + 1)
            if name == "error":
                try:
                    p = float(head.group(3))
                except (TypeError, ValueError):
                    raise ValueError(f"line {lineno}: error needs one probability, error(p)") from None
                prob.append(p)
                targets.append((det, obs))
        if sector_of_detector is None:
            sod = np.zeros(n_det, np.int64)
        else:
            sod = np.asarray(sector_of_detector, np.int64).ravel()
            if sod.size < n_det:
                raise ValueError(f"sector_of_detector has {sod.size} entries, the model uses {n_det} detectors")
            if sod.size and (sod.min() < 0 or sod.max() > 1):
                raise ValueError("sector_of_detector holds 0 or 1 per detector")
        nsec = 1 if sector_of_detector is None else 2
        local = np.zeros(sod.size, np.int64)
        counts, dmap = [], []
        for s in range(nsec):
            mine = np.flatnonzero(sod == s)
            local[mine] = np.arange(mine.size)
            counts.append(int(mine.size))
            dmap.append(mine)
        columns = []
        for det, obs in targets:
            det = np.asarray(det, np.int64)
            per = [local[det[sod[det] == s]] for s in range(nsec)]
            vis = [np.count_nonzero(np.unique(d, return_counts=True)[1] % 2) > 0 for d in per]
            columns.append([(per[s], obs if (vis[s] or (s == 0 and not any(vis))) else 0) for s in range(nsec)])
        return cls.from_columns(prob, columns, counts, (n_obs,) * nsec, detector_map=dmap, n_detectors=int(sod.size))

    def decoder_view(self, sector):
        """DecoderView of a sector: the explicit one when the model has it.  Otherwise derived: the mechanisms with p > 0, in index order, projected onto
        the sector (detector list, logical mask); projections without a detector are dropped (nothing to decode from); equal (detectors, logmask)
        projections merge into one column by p <- p (1 - q) + q (1 - p) in mechanism order (f64), columns in order of first appearance; the prior is
        prior_llrs(p_col)."""
        if self._views[sector] is not None:
            return self._views[sector]
        S = self.sectors[sector]
        cols, order = {}, []
        for l in np.flatnonzero(self.prob > 0):
            a, b = S.det_ptr[l], S.det_ptr[l + 1]
            if a == b:
                continue
            key = (S.det_idx[a:b].tobytes(), int(S.logmask[l]))
            q = float(self.prob[l])
            if key in cols:
                p = cols[key]
                cols[key] = p * (1.0 - q) + q * (1.0 - p)
            else:
                cols[key] = q
                order.append(key)
        n = len(order)
        dets = [np.frombuffer(key[0], np.uint16).astype(np.int64) for key in order]
        rows = np.concatenate(dets) if n else np.zeros(0, np.int64)
        colid = np.repeat(np.arange(n, dtype=np.int64), [d.size for d in dets]) if n else np.zeros(0, np.int64)
        by_row = np.argsort(rows, kind="stable")                       # columns were appended in ascending order: every row's columns stay sorted
        indptr = np.zeros(S.n_det + 1, np.int64)
        np.cumsum(np.bincount(rows, minlength=S.n_det), out=indptr[1:])
        view = DecoderView(indptr.astype(np.int32), colid[by_row].astype(np.int32), (S.n_det, n), prior_llrs(np.array([cols[key] for key in order], np.float64)),
                           np.array([key[1] for key in order], np.uint64))
        self._views[sector] = view
        return view

    def plan(self, graphs, max_iter=50, alphas=(1.0, 1.0), alpha_mode="dynamical", batch=16384, flags=0, use_osd=True, **kw):
        """A _lib.DemPlan of this model on `graphs` (one _lib.Graph of decoder_view(s) per sector)."""
        views = [self.decoder_view(s) for s in range(self.n_sectors)]
        return _lib.DemPlan(self.prob, [tuple(S) for S in self.sectors], list(graphs), [v.prior for v in views], [v.logmask for v in views], max_iter=max_iter,
                            alphas=alphas, alpha_mode=alpha_mode, batch=batch, flags=flags, use_osd=use_osd, **kw)


def _dem_rules(who, dem, maxIter, osd_order, alpha_mode, alvarado_alpha, decoder, relay_params, window, schedule, layers, decimation, precision, num_workers=None, lsd=None, correlated=None):
    """The argument rules run_dem_simulation and DemDecoder share, raised as ValueError before any device call -> (rules of engine._extension_rules,
    alpha_mode, (alpha of sector 0, alpha of sector 1))."""
    if not isinstance(dem, DetectorErrorModel):
        raise ValueError("dem must be a DetectorErrorModel (from_decoding_matrices, from_text, from_columns)")
    rules = engine._extension_rules(osd_order, precision, decimation, schedule, layers, window, decoder, relay_params, alpha_mode, alvarado_alpha, True, False,
                                    maxIter, num_workers, lsd=lsd, correlated=correlated)
    if rules.path == "correlated":
        if dem.n_sectors != 2:
            raise ValueError(f"{who}: correlated=... needs a detector error model with two sectors (this one has {dem.n_sectors})")
        from .correlated import links_from_dem
        rules.links = links_from_dem(dem, rules.correlated["mode"], rules.correlated["floor"])
    if decoder == "bp_osd" and osd_order > 0:
        raise ValueError(f"{who}: osd_order={osd_order} with decoder='bp_osd' asks for the OSD-w pass, which is not available on detector error "
                         "models; use decoder='bp_osd_cs' (osd_order is then the combination-sweep order)")
    if alpha_mode is None:
        alpha_mode = "dynamical"
    if alpha_mode not in ("dynamical", "alvarado"):
        raise ValueError(f"{who}: alpha_mode={alpha_mode!r} would run an alpha estimator, which draws errors at one error_rate; "
                         "use 'dynamical', or 'alvarado' with an explicit alvarado_alpha")
    if alpha_mode == "alvarado" and alvarado_alpha is None:
        raise ValueError(f"{who}: alpha_mode='alvarado' needs an explicit alvarado_alpha (the estimator draws errors at one error_rate)")
    if alpha_mode == "dynamical" and alvarado_alpha is not None:
        raise ValueError("alvarado_alpha is for alpha_mode='alvarado'")
    if alvarado_alpha is None:
        alphas = (1.0, 1.0)
    elif isinstance(alvarado_alpha, (list, tuple, np.ndarray)) and len(alvarado_alpha) == 2:
        alphas = (float(alvarado_alpha[0]), float(alvarado_alpha[1]))
    else:
        alphas = (float(alvarado_alpha),) * 2
    if rules.path == "window":
        for s, S in enumerate(dem.sectors):
            if S.layer_rows <= 0 or S.n_det % S.layer_rows:
                raise ValueError(f"window={window!r} needs the model's layer_rows (rows of one syndrome cycle): sector {s} has layer_rows={S.layer_rows} "
                                 f"for {S.n_det} detectors")
    if rules.path == "layered" and dem.n_sectors == 1 and rules.layers[1] is not None:
        raise ValueError("layers: the model has one sector, so the second row_layer must be None")
    return rules, alpha_mode, alphas


def run_dem_simulation(dem, num_trials=1000, maxIter=50, osd_order=0, alpha_mode=None, alvarado_alpha=None, base_seed=None, target_logical_errors=None,
                       max_trials=None, batch=16384, device=None, devices=None, num_workers=None, flags=0, decoder="bp_osd", relay_params=None, window=None,
                       schedule="flooding", layers=None, decimation=None, precision="f64", lsd=None, correlated=None, erasure=None, soft=None, post_select=None):
    """``run_simulation`` for a DetectorErrorModel: the same result keys, in-order early stop (``target_logical_errors``), ``num_workers`` / ``devices`` and
    extensions (``decoder`` with ``lsd`` and ``post_select`` for ``"bp_lsd"``, ``window``, ``schedule`` / ``layers``, ``decimation``, ``precision``, ``correlated`` with the links of
    ``correlated.links_from_dem``) under the same argument rules; sector 0 fills the ``z``
    keys, sector 1 the ``x`` keys (0 for a one-sector model).  ``window=(W, C)`` needs the model's ``layer_rows``.

    Out of scope (ValueError before any device call): the alpha / SCOPT estimators, which draw errors at one error rate -- use ``alpha_mode="dynamical"``
    (the default) or ``"alvarado"`` with an explicit ``alvarado_alpha`` (a number or a pair) -- and ``osd_order > 0`` with ``decoder="bp_osd"`` (the
    reference's OSD-w pass; ``decoder="bp_osd_cs"`` is the higher-order OSD of the fused pipeline) -- and ``erasure=...`` / ``soft=...``: heralded erasures and
    readout levels belong to gate locations, which a detector error model does not have."""
    if erasure is not None:
        raise ValueError("run_dem_simulation: erasure=... needs a circuit plan (run_simulation): a detector error model has no gate locations to erase")
    if soft is not None:
        raise ValueError("run_dem_simulation: soft=... needs a circuit plan (run_simulation): a detector error model has no measurement locations")
    rules, alpha_mode, alphas = _dem_rules("run_dem_simulation", dem, maxIter, osd_order, alpha_mode, alvarado_alpha, decoder, relay_params, window, schedule, layers,
                                           decimation, precision, num_workers, lsd=lsd, correlated=correlated)
    from .postselect import post_select_rules
    rules.post_select = post_select_rules("run_dem_simulation", post_select, decoder, target_logical_errors)
    rank, world, devices = engine._worker_devices(num_workers, devices, device)
    if base_seed is None:
        base_seed = int(np.random.randint(0, 2 ** 31))
    views = [dem.decoder_view(s) for s in range(dem.n_sectors)]
    graphs = [_lib.Graph(v.indptr, v.indices, v.shape[1], device=devices[0]) for v in views]

    def make_plan(own_graphs, dev):
        return dem.plan(own_graphs, max_iter=maxIter, alphas=alphas, alpha_mode=alpha_mode, batch=batch, flags=flags)

    return engine._run_trials(make_plan, graphs, [v.prior for v in views], [v.logmask for v in views], alphas[:dem.n_sectors], dem.k, rules, rank, world, devices,
                              base_seed, num_trials, max_trials, target_logical_errors, maxIter, osd_order, alpha_mode, batch, decoder, schedule, precision, {})


def read_b8(path, n_bits):
    """A file of bit-packed records (Stim's ``b8``: ceil(n_bits / 8) bytes per shot, bit d = (rec[d >> 3] >> (d & 7)) & 1) -> uint8[count, ceil(n_bits / 8)]."""
    width = (int(n_bits) + 7) // 8
    return np.fromfile(path, np.uint8).reshape(-1, width)


def _packed_events(events, n_detectors, bit_packed):
    """decode_batch's input rule -> bit-packed records uint8[count, >= ceil(n_detectors / 8)].  bool arrays are one detector per entry; uint8 arrays are
    told apart by their width when bit_packed is None (n_detectors wide: one detector per byte, values 0 / 1; ceil(n_detectors / 8) wide: packed)."""
    events = np.asarray(events)
    width = (n_detectors + 7) // 8
    if events.ndim != 2:
        raise ValueError(f"events must be [count, n_detectors] or bit-packed [count, {width}], got shape {events.shape}")
    if events.dtype == np.bool_:
        if bit_packed:
            raise ValueError("bit_packed=True needs uint8 records, got a bool array")
        bit_packed = False
    elif events.dtype != np.uint8:
        raise ValueError(f"events must be bool or uint8, got {events.dtype}")
    if bit_packed is None:
        fits = (events.shape[1] == n_detectors, events.shape[1] == width)
        if all(fits):
            raise ValueError(f"uint8 events of width {events.shape[1]} could be {n_detectors} detectors or {width} packed bytes: pass bit_packed=True or False")
        if not any(fits):
            raise ValueError(f"events are {events.shape[1]} wide: the model has {n_detectors} detectors ({width} bytes when bit-packed)")
        bit_packed = fits[1]
    if bit_packed:
        if events.shape[1] < width:
            raise ValueError(f"bit-packed events are {events.shape[1]} bytes wide: {n_detectors} detectors need {width}")
        return np.ascontiguousarray(events)
    if events.shape[1] != n_detectors:
        raise ValueError(f"events are {events.shape[1]} wide: the model has {n_detectors} detectors")
    if events.dtype == np.uint8 and events.size and events.max() > 1:
        raise ValueError("unpacked uint8 events hold 0 or 1 per detector")
    return _lib.pack_events(events)


class DemDecoder:
    """Decodes recorded detection events of a DetectorErrorModel on the fused device pipeline: events -> decode -> OSD -> predict
    (``qldpc_circuit_plan_decode_events``), the ``decode_batch`` of other DEM decoders.  The arguments are ``run_dem_simulation``'s, under the same rules
    (ValueError before any device call); the plan is created on the first decode.

    Events come in the MODEL's detector numbering (``dem.detector_map``; for ``from_text`` the text's ``D<i>``), ``dem.n_detectors`` per shot.  ``seed`` and
    the global shot index (``shot_begin`` + row) are what Relay-BP draws from; every other decoder ignores them.  So a prediction is a function of
    (record, seed, shot index) and depends neither on ``batch`` nor on how the shots are split over calls.

    ``confidence`` (with ``decoder="bp_lsd"``; a kind of ``simulation.postselect.KINDS``) makes ``decode_batch(events, return_confidence=True)`` return
    a score uint64[count] beside the predictions: small = trustworthy, 2^64 - 1 = LSD made no statement (``qldpc_circuit_plan_use_confidence``; the
    weights are ``_lib.quantise_weights`` of the decoder views' priors)."""

    def __init__(self, dem, maxIter=50, decoder="bp_osd", osd_order=0, window=None, schedule="flooding", layers=None, decimation=None, precision="f64",
                 relay_params=None, alpha_mode=None, alvarado_alpha=None, batch=16384, device=None, seed=0, flags=0, lsd=None, correlated=None,
                 confidence=None):
        self._rules, self._alpha_mode, self._alphas = _dem_rules("DemDecoder", dem, maxIter, osd_order, alpha_mode, alvarado_alpha, decoder, relay_params, window,
                                                                 schedule, layers, decimation, precision, lsd=lsd, correlated=correlated)
        if int(batch) < 1:
            raise ValueError("batch must be >= 1")
        if confidence is not None:
            from .postselect import post_select_rules
            self._rules.post_select = post_select_rules("DemDecoder", {"kind": confidence, "edges": []}, decoder)
        self.dem, self.seed, self.batch, self.device = dem, int(seed), int(batch), device
        self._max_iter, self._osd_order, self._flags = maxIter, osd_order, flags
        self._plan = self._graphs = None

    def _ensure_plan(self):
        if self._plan is None:
            dem = self.dem
            dev = 0 if self.device is None else int(self.device)
            views = [dem.decoder_view(s) for s in range(dem.n_sectors)]
            if self._rules.post_select is not None:
                self._rules.post_select["weights"] = [_lib.quantise_weights(v.prior) for v in views]
            switch, _ = engine._plan_switch(self._rules, [(v.indptr, v.indices, v.shape[1]) for v in views], self._osd_order)
            self._graphs = [_lib.Graph(v.indptr, v.indices, v.shape[1], device=dev) for v in views]
            plan = dem.plan(self._graphs, max_iter=self._max_iter, alphas=self._alphas, alpha_mode=self._alpha_mode, batch=self.batch, flags=self._flags)
            try:
                switch(plan)
                plan.set_event_layout(dem.n_detectors, *dem.detector_map)
            except Exception:
                plan.close()
                raise
            self._plan = plan
        return self._plan

    def decode_to_flags(self, events, bit_packed=None, shot_begin=0, return_confidence=False):
        """decode_batch and the flags uint8[count]: bit 0 / 1 = converged, 2 / 3 = the correction does not reproduce the syndrome, 4 / 5 = zero syndrome,
        of sector 0 / 1; with return_confidence a third entry, the score uint64[count]."""
        if return_confidence and self._rules.post_select is None:
            raise ValueError("return_confidence=True needs DemDecoder(..., decoder='bp_lsd', confidence=<kind>)")
        packed = _packed_events(events, self.dem.n_detectors, bit_packed)
        if int(shot_begin) < 0:
            raise ValueError("shot_begin must be >= 0")
        pred = self._ensure_plan().decode_events(packed, seed=self.seed, shot_begin=int(shot_begin), scores=bool(return_confidence))
        out = tuple(((pred[s][:, None] >> np.arange(k, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool) for s, k in enumerate(self.dem.k))
        out = out[0] if self.dem.n_sectors == 1 else out
        return (out, pred[2], pred[3]) if return_confidence else (out, pred[2])

    def decode_batch(self, events, bit_packed=None, shot_begin=0, return_confidence=False):
        """events: bool or uint8 [count, n_detectors] (0 / 1 per detector), or bit-packed uint8 [count, ceil(n_detectors / 8)] (``_lib.pack_events``,
        ``read_b8``); bit_packed None = told apart by dtype and width.  Returns the predicted observable flips bool[count, k] per sector -- a pair for a
        two-sector model, the array itself for a one-sector model (column r = ``L<r>`` of the text).  return_confidence=True (a decoder created with
        ``confidence=``): (predictions, score uint64[count])."""
        res = self.decode_to_flags(events, bit_packed, shot_begin, return_confidence)
        return (res[0], res[2]) if return_confidence else res[0]

    def close(self):
        if self._plan is not None:
            self._plan.close()
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
