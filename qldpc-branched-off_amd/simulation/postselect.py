"""Post-selection on the confidence of BP+LSD: discard the trials the decoder is unsure of and ask what logical error rate is left at what abort rate.

A circuit or detector-error-model plan with ``use_confidence`` scores every trial from the cluster statistics of its LSD stage (small = trustworthy;
the laws are in include/qldpc_hip.h at qldpc_lsd_stats_batch and qldpc_circuit_plan_use_confidence) and counts hist[bin][outcome] on the device,
bin = the number of edges <= score and outcome = bit0 z_err | bit1 x_err.  ``PostSelection`` holds such a histogram and turns it into the curve;
``run_simulation(decoder="bp_lsd", post_select={"kind": ..., "edges": ...})`` and ``run_dem_simulation`` return one as ``result["post_selection"]``.

A cut k accepts the trials in the bins below k: cut 0 accepts nothing, cut nbins everything.  The last bin always holds the trials LSD made no
statement about (score 2^64 - 1: capped, or without candidates), so every cut but the last aborts them."""
import math

import numpy as np

from .. import _lib

KINDS = tuple(sorted(_lib.CONF_KINDS, key=_lib.CONF_KINDS.get))

# default_edges: the score a ladder reaches (a power of two) and its steps per octave.  The squared norms get half the steps, which is the same
# resolution in the norm itself.  cols_*: a cluster holds fewer than 2^16 columns; llr_*: weights are uint16 and their sum stays below 2^32.
_LADDER = {"cols_1": (16, 4), "cols_2": (32, 2), "cols_inf": (16, 4), "llr_1": (32, 4), "llr_2": (62, 2), "llr_inf": (32, 4)}


def default_edges(kind, steps_per_octave=None, top_bits=None):
    """The default bin edges of a kind: the geometric ladder ceil(2^(i / s)), i = 0 .. top_bits * s, without repeats (uint64, strictly increasing).
    Its first edge is 1, so bin 0 holds exactly the trials with no cluster at all (score 0: both sectors converged or had zero residual), and a score
    beyond the last edge 2^top_bits, "no statement" among them, falls in the last bin.  s = steps_per_octave and top_bits default per kind (_LADDER).
    Computed in integers (ceil(2^(i / s)) for s = 1, 2, 4 by integer square roots), so the edges are the same on every machine."""
    kind = KINDS[_lib.conf_kind(kind)]
    bits, steps = _LADDER[kind]
    steps = steps if steps_per_octave is None else int(steps_per_octave)
    bits = bits if top_bits is None else int(top_bits)
    if steps not in (1, 2, 4):
        raise ValueError(f"steps_per_octave must be 1, 2 or 4, got {steps_per_octave!r}")
    if not 0 <= bits <= 63:
        raise ValueError(f"top_bits must be in 0..63, got {top_bits!r}")
    edges = []
    for i in range(bits * steps + 1):
        root = 1 << i                                                            # floor(2^(i / steps)): nested integer square roots are exact
        for _ in range(steps.bit_length() - 1):
            root = math.isqrt(root)
        e = root if root ** steps == 1 << i else root + 1
        if not edges or e > edges[-1]:
            edges.append(e)
    return np.array(edges, np.uint64)


class PostSelection:
    """A histogram of (score bin, outcome) and what post-selection on it gives.  hist: uint64[nbins, 4]; edges: uint64[nbins - 1]; kind: a name of KINDS."""

    def __init__(self, hist, edges, kind):
        self.kind = KINDS[_lib.conf_kind(kind)]
        self.edges = _lib.conf_edges(edges)
        self.hist = np.ascontiguousarray(hist, np.uint64)
        if self.hist.shape != (self.edges.size + 1, 4):
            raise ValueError(f"hist must be uint64[{self.edges.size + 1}, 4] for {self.edges.size} edges, got shape {self.hist.shape}")

    @property
    def trials(self):
        return int(self.hist.sum(dtype=np.uint64))

    def __add__(self, other):
        if not isinstance(other, PostSelection) or other.kind != self.kind or not np.array_equal(other.edges, self.edges):
            raise ValueError("only histograms of the same kind and edges add")
        return PostSelection(self.hist + other.hist, self.edges, self.kind)

    def curve(self):
        """For every cut k = 0 .. nbins (accept the trials in bins < k), as arrays of nbins + 1 entries: cut, accepted, failures, failures_z, failures_x
        (int64), abort_rate = 1 - accepted / trials, ler = failures / accepted and its binomial std_error = sqrt(ler (1 - ler) / accepted) (float64;
        nan where nothing is accepted).  threshold[k]: the scores a cut accepts are those below it (edges[k - 1]; 0 for cut 0, 2^64 for the last cut,
        as Python integers)."""
        h = self.hist.astype(np.int64)
        zero = np.zeros((1, 4), np.int64)
        cum = np.concatenate([zero, np.cumsum(h, axis=0)])
        accepted = cum.sum(axis=1)
        failures = cum[:, 1] + cum[:, 2] + cum[:, 3]
        total = int(accepted[-1])
        with np.errstate(divide="ignore", invalid="ignore"):
            ler = np.where(accepted > 0, failures / accepted, np.nan)
            err = np.where(accepted > 0, np.sqrt(ler * (1.0 - ler) / accepted), np.nan)
            abort = 1.0 - accepted / total if total else np.full(accepted.shape, np.nan)
        return {"cut": np.arange(h.shape[0] + 1), "threshold": [0] + [int(e) for e in self.edges] + [1 << 64], "accepted": accepted, "failures": failures,
                "failures_z": cum[:, 1] + cum[:, 3], "failures_x": cum[:, 2] + cum[:, 3], "abort_rate": abort, "ler": ler, "std_error": err}

    def at_abort_rate(self, x):
        """The working point for an abort budget x in [0, 1]: of the cuts that abort at most x of the trials, the one that aborts most (the abort rate
        does not grow with the cut, and the last cut aborts nothing, so there is one) -> a dict with that cut's entry of every array of curve()."""
        x = float(x)
        if not 0.0 <= x <= 1.0:
            raise ValueError(f"abort rate {x!r} outside 0..1")
        c = self.curve()
        if self.trials == 0:
            k = self.hist.shape[0]
        else:
            k = int(np.flatnonzero(c["abort_rate"] <= x + 1e-12)[0])
        return {name: (v[k] if isinstance(v, list) else v[k].item()) for name, v in c.items()}

    def no_statement(self):
        """The trials of the last bin: with edges below 2^64 - 1 it holds every trial LSD made no statement about (and the scores beyond the last edge)."""
        return int(self.hist[-1].sum(dtype=np.uint64))


def post_select_rules(who, post_select, decoder, target_logical_errors=None):
    """The argument rules of ``post_select=``: None, or a dict with kind (a name of KINDS) and, optionally, edges (None: default_edges(kind)) ->
    {"kind": name, "edges": uint64[nbins - 1]} or None.  ValueError before any device call."""
    if post_select is None:
        return None
    if decoder != "bp_lsd":
        raise ValueError(f"{who}: post_select=... is for decoder='bp_lsd' (the confidence is the cluster statistics of LSD), got decoder={decoder!r}")
    if target_logical_errors is not None and target_logical_errors > 0:
        raise ValueError(f"{who}: post_select=... does not go with target_logical_errors (the in-order cut and a device-side histogram do not compose)")
    if not isinstance(post_select, dict) or "kind" not in post_select:
        raise ValueError(f"{who}: post_select must be a dict with kind and, optionally, edges (or None)")
    unknown = set(post_select) - {"kind", "edges"}
    if unknown:
        raise ValueError(f"{who}: unknown post_select parameter(s): {sorted(unknown)}")
    if not isinstance(post_select["kind"], str):
        raise ValueError(f"{who}: post_select['kind'] must be one of {list(KINDS)}")
    kind = KINDS[_lib.conf_kind(post_select["kind"])]
    edges = post_select.get("edges")
    return {"kind": kind, "edges": default_edges(kind) if edges is None else _lib.conf_edges(edges)}
