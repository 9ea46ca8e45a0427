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
    of one syndrome cycle, for ``window=``).  ``views``: an explicit DecoderView per sector, or None to derive it."""

    def __init__(self, prob, sectors, views=None):
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
        """The one-sector model that keeps sector s alone (every mechanism stays, so the draws of a trial do not change)."""
        return DetectorErrorModel(self.prob, [self.sectors[s]], [self._views[s]])

    @classmethod
    def from_columns(cls, prob, columns, n_det, k, layer_rows=None, views=None):
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
        return cls(prob, sectors, views)

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
        targets: an undetectable logical flip) counts in sector 0.  With one sector that is the usual memory experiment."""
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
        counts = []
        for s in range(nsec):
            mine = np.flatnonzero(sod == s)
            local[mine] = np.arange(mine.size)
            counts.append(int(mine.size))
        columns = []
        for det, obs in targets:
            det = np.asarray(det, np.int64)
            per = [local[det[sod[det] == s]] for s in range(nsec)]
            vis = [np.count_nonzero(np.unique(d, return_counts=True)[1] % 2) > 0 for d in per]
            columns.append([(per[s], obs if (vis[s] or (s == 0 and not any(vis))) else 0) for s in range(nsec)])
        return cls.from_columns(prob, columns, counts, (n_obs,) * nsec)

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


def run_dem_simulation(dem, num_trials=1000, maxIter=50, osd_order=0, alpha_mode=None, alvarado_alpha=None, base_seed=None, target_logical_errors=None,
                       max_trials=None, batch=16384, device=None, devices=None, num_workers=None, flags=0, decoder="bp_osd", relay_params=None, window=None,
                       schedule="flooding", layers=None, decimation=None, precision="f64"):
    """``run_simulation`` for a DetectorErrorModel: the same result keys, in-order early stop (``target_logical_errors``), ``num_workers`` / ``devices`` and
    extensions (``decoder``, ``window``, ``schedule`` / ``layers``, ``decimation``, ``precision``) under the same argument rules; sector 0 fills the ``z``
    keys, sector 1 the ``x`` keys (0 for a one-sector model).  ``window=(W, C)`` needs the model's ``layer_rows``.

    Out of scope (ValueError before any device call): the alpha / SCOPT estimators, which draw errors at one error rate -- use ``alpha_mode="dynamical"``
    (the default) or ``"alvarado"`` with an explicit ``alvarado_alpha`` (a number or a pair) -- and ``osd_order > 0`` with ``decoder="bp_osd"`` (the
    reference's OSD-w pass; ``decoder="bp_osd_cs"`` is the higher-order OSD of the fused pipeline)."""
    if not isinstance(dem, DetectorErrorModel):
        raise ValueError("dem must be a DetectorErrorModel (from_decoding_matrices, from_text, from_columns)")
    rules = engine._extension_rules(osd_order, precision, decimation, schedule, layers, window, decoder, relay_params, alpha_mode, alvarado_alpha, True, False,
                                    maxIter, num_workers)
    if decoder == "bp_osd" and osd_order > 0:
        raise ValueError(f"run_dem_simulation: osd_order={osd_order} with decoder='bp_osd' asks for the OSD-w pass, which is not available on detector error "
                         "models; use decoder='bp_osd_cs' (osd_order is then the combination-sweep order)")
    if alpha_mode is None:
        alpha_mode = "dynamical"
    if alpha_mode not in ("dynamical", "alvarado"):
        raise ValueError(f"run_dem_simulation: alpha_mode={alpha_mode!r} would run an alpha estimator, which draws errors at one error_rate; "
                         "use 'dynamical', or 'alvarado' with an explicit alvarado_alpha")
    if alpha_mode == "alvarado" and alvarado_alpha is None:
        raise ValueError("run_dem_simulation: alpha_mode='alvarado' needs an explicit alvarado_alpha (the estimator draws errors at one error_rate)")
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
    rank, world, devices = engine._worker_devices(num_workers, devices, device)
    if base_seed is None:
        base_seed = int(np.random.randint(0, 2 ** 31))
    views = [dem.decoder_view(s) for s in range(dem.n_sectors)]
    graphs = [_lib.Graph(v.indptr, v.indices, v.shape[1], device=devices[0]) for v in views]

    def make_plan(own_graphs, dev):
        return dem.plan(own_graphs, max_iter=maxIter, alphas=alphas, alpha_mode=alpha_mode, batch=batch, flags=flags)

    return engine._run_trials(make_plan, graphs, [v.prior for v in views], [v.logmask for v in views], alphas[:dem.n_sectors], dem.k, rules, rank, world, devices,
                              base_seed, num_trials, max_trials, target_logical_errors, maxIter, osd_order, alpha_mode, batch, decoder, schedule, precision, {})
