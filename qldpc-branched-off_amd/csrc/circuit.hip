// Circuit-level Monte-Carlo (BASELINE config 5): run_trial_fast (reference src/noise/simulation.py:21-107) and the
// per-trial pipeline _run_single_trial_fast (src/simulation/engine.py:68-122), batched on the device.
//
// MI355X-first formulation.  The reference builds a noisy op list per trial and walks ~20k ops twice.  Pauli-frame
// propagation is linear over GF(2) in the inserted faults, so here the effect of ONE flip at every (error location,
// qubit slot) -- its detector flips and logical flips, per sector -- is computed once per plan by a batched frame
// simulation (one lane per single-fault circuit; the same thing the reference's builder.py:37-51 does to build H).
// A trial is then: draw the faulty locations (Philox), XOR the signatures of their Pauli components into a bit-set in
// LDS.  Equality with the literal simulation is asserted against the CPU checker on identical random draws.
// Random draws of trial g: location l faulty iff word (l&3) of Philox(g, block l>>2, domain 1) < thr; its Pauli choice
// is word 0 of Philox(g, l, domain 2) mod 3 (IDLE, noise/kernels.py:260-272) or mod 15 (CNOT, :274-344).
#include "common.h"
#include "launchers.h"
#include "clocks.h"
#include "sampler_common.h"
#include "judge.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace qldpc {

// ---- single-fault frame simulation: lane = (location, slot); ops shared; frames laid out [qubit][lane] ----
template <bool XSECTOR>
__global__ void fault_signature_kernel(int nl, const int32_t *__restrict__ lane_pos, const int8_t *__restrict__ lane_after,
                                       const int32_t *__restrict__ lane_qubit, int64_t len, const int32_t *__restrict__ ops,
                                       const int32_t *__restrict__ q1, const int32_t *__restrict__ q2, int tq, int nsyn,
                                       int8_t *__restrict__ state, int8_t *__restrict__ hist) {
    const int lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= nl) return;
    for (int q = 0; q < tq; q++) state[(size_t)q * nl + lane] = 0;
    const int pos = lane_pos[lane], fq = lane_qubit[lane];
    const bool after = lane_after[lane] != 0;
    int sc = 0;
    for (int64_t i = 0; i < len; i++) {
        const int op = ops[i], a = q1[i], c = q2[i];
        if (i == pos && !after && fq >= 0) state[(size_t)fq * nl + lane] ^= 1;       // Meas: flip BEFORE (kernels.py:210-221)
        if (op == C_OP_CNOT) {
            if (!XSECTOR) state[(size_t)a * nl + lane] ^= state[(size_t)c * nl + lane];   // Z: target -> control (kernels.py:55-57)
            else state[(size_t)c * nl + lane] ^= state[(size_t)a * nl + lane];            // X: control -> target (kernels.py:136-138)
        } else if (op == (XSECTOR ? C_OP_PREP_Z : C_OP_PREP_X)) {
            state[(size_t)a * nl + lane] = 0;
        } else if (op == (XSECTOR ? C_OP_MEAS_Z : C_OP_MEAS_X)) {
            if (sc < nsyn) hist[(size_t)sc * nl + lane] = state[(size_t)a * nl + lane];
            sc++;
        }
        if (i == pos && after && fq >= 0) state[(size_t)fq * nl + lane] ^= 1;        // Prep/CNOT: flip AFTER (kernels.py:236-258,274)
    }
}

// the independent draws in the frame of sampler_common.h: a lane per Philox block = four locations, a faulty one fires its components
__global__ __launch_bounds__(256) void circuit_sample_kernel(int64_t B, int64_t trial_begin, uint32_t seed_lo, uint32_t seed_hi, uint32_t thr,
                                                             int n_locs, const uint8_t *__restrict__ loc_type, SigTab Z, SigTab X, SampleOut O) {
    extern __shared__ uint32_t sm[];
    const int nblk = (n_locs + 3) >> 2;
    sample_trials<true>(sm, B, trial_begin, O, 0, nullptr, [&](int64_t, uint64_t g, const SampleLds &L) {
        for (int blk = threadIdx.x; blk < nblk; blk += blockDim.x) {
            uint32_t o[4];
            philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)blk, 1u, seed_lo, seed_hi, o);
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int l = 4 * blk + w;
                if (l < n_locs && o[w] < thr) fire_location(Z, X, loc_type, g, l, seed_lo, seed_hi, L.b0, L.b1, L.lacc);
            }
        }
    });
}

// per trial (32 lanes): decoded logical action H_logical @ det (engine.py:99,119) (judge.h) vs the true logical flips, both sectors
// TWO = false: a one-sector plan (a detector error model with n_sectors = 1): X is not read, its slots and outcome bit 1 stay 0
template <bool SPARSE, bool TWO>
__global__ __launch_bounds__(256) void circuit_judge_kernel(int64_t B, JudgeSector Z, JudgeSector X, unsigned long long *__restrict__ tally,
                                                            uint8_t *__restrict__ outcome, const int32_t *__restrict__ fail_counts) {
    __shared__ unsigned long long acc[QLDPC_TALLY_SLOTS];
    __shared__ uint32_t parbits[SPARSE ? 8 * 2 * 128 : 1];                      // per trial of the workgroup: the two sectors' parity bits (m <= 4096)
    if (threadIdx.x < QLDPC_TALLY_SLOTS) acc[threadIdx.x] = 0ull;
    __syncthreads();
    if (fail_counts && blockIdx.x == 0 && threadIdx.x == 0) {                 // OSD-0 calls of this batch = its BP failures per sector
        acc[QLDPC_TALLY_OSD_Z] = (unsigned long long)fail_counts[0];
        if (TWO) acc[QLDPC_TALLY_OSD_X] = (unsigned long long)fail_counts[4];
    }
    __syncthreads();
    const int lane = threadIdx.x & 31;
    const int64_t b = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (b < B) {
        bool ze, zn, zb, xe = false, xn = false, xb = false;
        if (SPARSE) {
            uint32_t *par = parbits + (threadIdx.x >> 5) * 256;
            ze = judge_sector_sparse(Z, b, lane, par, zn, zb) != Z.true_log[b];
            if (TWO) xe = judge_sector_sparse(X, b, lane, par + 128, xn, xb) != X.true_log[b];
        } else {
            ze = judge_sector(Z, b, lane, zn, zb) != Z.true_log[b];
            if (TWO) xe = judge_sector(X, b, lane, xn, xb) != X.true_log[b];
        }
        if (lane == 0) {
            if (outcome) outcome[b] = (uint8_t)((ze ? 1 : 0) | (xe ? 2 : 0));               // (z_err, x_err) of engine.py:117-122
            atomicAdd(&acc[QLDPC_TALLY_TRIALS], 1ull);
            if (ze) atomicAdd(&acc[QLDPC_TALLY_Z_ERR], 1ull);
            if (xe) atomicAdd(&acc[QLDPC_TALLY_X_ERR], 1ull);
            if (ze || xe) atomicAdd(&acc[QLDPC_TALLY_TOTAL_ERR], 1ull);                       // engine.py:122
            if (Z.conv[b]) atomicAdd(&acc[QLDPC_TALLY_BP_CONV_Z], 1ull);
            if (TWO && X.conv[b]) atomicAdd(&acc[QLDPC_TALLY_BP_CONV_X], 1ull);
            atomicAdd(&acc[QLDPC_TALLY_ITERS_Z], (unsigned long long)(Z.iters[b] + 1));
            if (TWO) atomicAdd(&acc[QLDPC_TALLY_ITERS_X], (unsigned long long)(X.iters[b] + 1));
            if (!zn) atomicAdd(&acc[QLDPC_TALLY_ZERO_SYND_Z], 1ull);
            if (TWO && !xn) atomicAdd(&acc[QLDPC_TALLY_ZERO_SYND_X], 1ull);
            if (zb) atomicAdd(&acc[QLDPC_TALLY_UNSAT_Z], 1ull);
            if (xb) atomicAdd(&acc[QLDPC_TALLY_UNSAT_X], 1ull);
        }
    }
    __syncthreads();
    if (threadIdx.x < QLDPC_TALLY_SLOTS && acc[threadIdx.x]) atomicAdd(&tally[threadIdx.x], acc[threadIdx.x]);
}

__global__ void collect_failed2_kernel(int64_t B, const uint8_t *__restrict__ conv, int32_t *__restrict__ list, int32_t *__restrict__ count) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && !conv[b]) list[atomicAdd(count, 1)] = (int32_t)b;
}

}  // namespace qldpc

using namespace qldpc;

// What both sectors decode with, on two axes; a plan is created as FLOOD + OSD0 and qldpc_circuit_plan_use_* moves it (switch_allowed holds the rules).
enum class Path { FLOOD, LAYERED, DECIM, F32, RELAY, WINDOW, CORRELATED, ERASURE, SOFT };      // who fills the BP bracket and its follow-up
enum class Osd { OSD0, CS, LSD };                                     // the OSD stage of a plan that has one (use_osd, and a path other than RELAY)
// What a trial is drawn with, the third axis (sampler_switch_allowed holds its rules; only launch_sampler and the two record exports read it).  A plan is
// created on INDEPENDENT: every location of a circuit at the plan's p (circuit.hip), or every mechanism of a detector error model at its own probability
// (dem.hip; `dem` is a property of the plan, the source of its tables, and no switch).  FIXED_WEIGHT: exactly `fixed_weight` faults per trial
// (fixed_weight.hip).  ERASURE: heralded erasures at `ethr` on top of the independent draws (erasure.hip).  NOISE_MODEL: a threshold per location
// class and weighted Paulis, `nm`, in place of p and r % K (noise_model.hip).  SOFT: a confidence level and a flip per measurement, `sr`, on top of the
// independent draws (soft.hip).  A sampler's parameters and buffers outlive a switch away from it; they are read only while the plan is on it.
enum class Sampler { INDEPENDENT, FIXED_WEIGHT, ERASURE, NOISE_MODEL, SOFT };

struct qldpc_circuit_plan {
    // Everything that exists once per sector: sec[0] = Z, sec[1] = X.  A batch decodes Z, then X, on the caller's stream.
    struct Sector {
        const qldpc_graph *g = nullptr;
        int nsyn = 0, layer_rows = 0;              // detectors (= rows of g); rows per syndrome cycle
        // on the host: the prior lets the decode dispatch pick the LDS-resident workgroup kernel (minsum_wg2.hip), the window decoder takes both at the switch
        std::vector<double> h_prior, h_alpha;
        DevBuf d_ptr, d_idx, d_log;                // fault signatures (SigTab)
        DevBuf d_alpha, d_prior, d_lm;
        DevBuf d_syn, d_true, d_det, d_llr, d_conv, d_iter, d_list;
        DevBuf d_legs;                             // Path::RELAY: legs per trial; Path::DECIM: rounds per trial
        DevBuf d_flips;                            // Osd::CS: workspace of the sweep
        DevBuf d_lsd_info;                         // Osd::LSD: info of the batch in flight
        // ... with qldpc_circuit_plan_use_confidence: the cluster statistics uint64[batch][8] of the batch in flight (zeroed, then the unconverged
        // shots' rows from lsd_kernel), and the weight table uint16[n] of the sector (has_conf_w: one was given)
        DevBuf d_lsd_stats, d_conf_w;
        bool has_conf_w = false;
        // decode of recorded events (events.hip): the record bit of every row (ev_tab, else the contiguous run at ev_base); the predictions of a batch
        DevBuf d_evtab, d_pred;
        // Path::ERASURE (erasure.hip): the sector's tables location -> (column, h) and column -> lut run; the per-shot prior f64[batch][n] of a batch
        DevBuf d_er_ptr, d_er_col, d_er_h, d_er_lutptr, d_er_lut, d_eprior;
        // Path::SOFT (soft.hip): the sector's tables measurement -> (column, weight) and column -> lut run; its per-shot prior shares d_eprior
        DevBuf d_so_col, d_so_w, d_so_lutptr, d_so_lut;
        bool ev_tab = false;
        int ev_base = 0;
        // the decoder objects of a path, below the buffers they write so that they go first (each waits for what it has in flight)
        Handle<qldpc_window_decoder, qldpc_window_decoder_destroy> win;       // Path::WINDOW (window.hip)
        Handle<qldpc_layered_decoder, qldpc_layered_decoder_destroy> lay;     // Path::LAYERED (minsum_layered.hip)
        Handle<qldpc_minsum32_decoder, qldpc_minsum32_decoder_destroy> f32;   // Path::F32 (minsum_f32.hip)
    } sec[2];
    int device = 0, k = 0, n_locs = 0, max_iter = 0, use_osd = 0, flags = 0;
    int nsec = 2, ks[2] = {0, 0};                  // sectors in use (1: a one-sector detector error model, sec[1] stays empty); logicals per sector
    // dem: the sampler draws from a detector error model (dem.hip).  n_locs then counts its mechanisms, d_ptr / d_idx / d_log of a sector hold their
    // projection onto it, and d_thr their thresholds (uint32, zero-padded to a multiple of four).
    bool dem = false;
    DevBuf d_thr;
    Sampler sampler = Sampler::INDEPENDENT;
    // Sampler::FIXED_WEIGHT: faults per trial.  dem_odd: the first mechanism whose threshold differs from mechanism 0's (-1: none), which refuses the switch
    int fixed_weight = 0;
    int64_t dem_odd = -1;
    // Sampler::ERASURE: the threshold per op code; d_erased: the herald record uint32[batch][ceil(n_locs / 32)] of a batch
    uint32_t ethr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    DevBuf d_erased;
    double era_alpha = 1.0;                        // Path::ERASURE: constant alpha
    double p = 0, damping = 1, clip = 20;
    uint32_t thr = 0;
    int64_t batch = 0;
    bool nanfree = false;
    DevBuf d_loc_type, d_count, d_tally, d_outcome, d_clk;     // d_count: [0] Z failures, [4] X failures (int32, 16 bytes apart)
    int ev_bits = 0;                               // bits of an event record that rows may name; 0: the default layout (sector 0's rows, then sector 1's)
    DevBuf d_events, d_evflags;                    // qldpc_circuit_plan_decode_events: the records of a batch (staging), its flags
    Path path = Path::FLOOD;
    Osd osd = Osd::OSD0;
    RelayParams rp{};                              // Path::RELAY (relay_bp.hip)
    DecimParams dp{};                              // Path::DECIM (decimation.hip)
    // Path::CORRELATED (shot_prior.hip): constant alpha; the links sector-0 column -> sector-1 column; base_x in place of sector 1's prior (corr_base)
    double corr_alpha = 1.0;
    bool corr_base = false;
    DevBuf d_cl_ptr, d_cl_src, d_cl_llr, d_cl_base;
    int cs_order = 0;                              // Osd::CS (osd_cs.hip)
    int lsd_bits = 0, lsd_rows = 0;                // Osd::LSD (lsd.hip)
    DevBuf d_lsd_counts;                           // ... uint64[2][3]: shots per sector that ended with flag 0 / 1 / 2 (the kernel accumulates)
    // qldpc_circuit_plan_use_confidence (confidence.hip): conf_kind -1 = off, else QLDPC_CONF_*; d_score: uint64[batch] of the batch in flight; d_edges:
    // uint64[conf_bins - 1]; d_hist: uint64[conf_bins][4], accumulated by every run until it is read with clear
    int conf_kind = -1, conf_bins = 0;
    DevBuf d_score, d_edges, d_hist;
    // hipEvent brackets of the phases of every batch not yet read by qldpc_circuit_plan_phase_times
    struct Bracket { int phase; hipEvent_t a, b; };
    std::vector<Bracket> pending;
    std::vector<hipEvent_t> pool;
    double phase_ms[QLDPC_CIRCUIT_PHASES] = {0, 0, 0, 0, 0, 0};
    int64_t batches = 0;
    // Sampler::NOISE_MODEL: the checked model; d_loc_cls: the op codes of d_loc_type, four to a word (uploaded at the first switch that reads them)
    NoiseModelHost nm{};
    DevBuf d_loc_cls;
    // Sampler::SOFT: the checked readout channel; n_meas: the MeasX / MeasZ locations (-1 until soft_prepare counts them); d_meas_rank: a location's rank
    // among them; d_levels: the level record uint8[batch][n_meas] of a batch
    SoftReadoutHost sr{};
    int n_meas = -1;
    DevBuf d_meas_rank, d_levels;
    double soft_alpha = 1.0;                       // Path::SOFT: constant alpha
    int soft_levels = 0;                           // Path::SOFT: the K its tables were built for
    int32_t *fail_count(int sector) { return d_count.as<int32_t>() + 4 * sector; }
    bool osd_stage() const { return use_osd && path != Path::RELAY; }            // the judge then adds d_count to the OSD tally slots
    ~qldpc_circuit_plan() {                        // the events; the sectors' decoder objects and every buffer then release themselves
        (void)hipSetDevice(device);
        for (auto &br : pending) { (void)hipEventDestroy(br.a); if (br.b) (void)hipEventDestroy(br.b); }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
};
using Sector = qldpc_circuit_plan::Sector;
static const int kPhaseBp[2] = {QLDPC_PHASE_BP_Z, QLDPC_PHASE_BP_X}, kPhaseOsd[2] = {QLDPC_PHASE_OSD_Z, QLDPC_PHASE_OSD_X};

static hipEvent_t plan_event(qldpc_circuit_plan *P) {
    if (!P->pool.empty()) { hipEvent_t e = P->pool.back(); P->pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
}
// brackets `phase` on stream s: call once before (open = true) and once after the launches
static int phase_mark(qldpc_circuit_plan *P, int phase, hipStream_t s, bool open) {
    hipEvent_t e = plan_event(P);
    if (!e) { set_error("hipEventCreate failed"); return QLDPC_ERR_HIP; }
    QLDPC_HIP_TRY(hipEventRecord(e, s));
    if (open) P->pending.push_back({phase, e, nullptr});
    else {
        for (auto it = P->pending.rbegin(); it != P->pending.rend(); ++it)
            if (it->phase == phase && it->b == nullptr) { it->b = e; return QLDPC_OK; }
        P->pool.push_back(e);
    }
    return QLDPC_OK;
}

// Folds finished phase brackets into phase_ms and hands their events back to the pool; every entry leaves `pending` before its events enter the
// pool (an entry is never in both).  wait = false: only brackets whose closing event has already completed (no host wait).
static void drain_phases(qldpc_circuit_plan *P, bool wait) {
    size_t keep = 0;
    for (size_t i = 0; i < P->pending.size(); i++) {
        const qldpc_circuit_plan::Bracket br = P->pending[i];
        if (!br.b) {                                       // an opener whose launches failed before the closing mark
            if (wait) P->pool.push_back(br.a); else P->pending[keep++] = br;
            continue;
        }
        const bool done = wait ? (hipEventSynchronize(br.b) == hipSuccess) : (hipEventQuery(br.b) == hipSuccess);
        if (!done && !wait) { P->pending[keep++] = br; continue; }
        float t = 0;
        if (done && hipEventElapsedTime(&t, br.a, br.b) == hipSuccess) P->phase_ms[br.phase] += t;
        P->pool.push_back(br.a); P->pool.push_back(br.b);
    }
    P->pending.resize(keep);
    (void)hipGetLastError();                               // hipEventQuery's hipErrorNotReady is not an error of the caller
}

// What the descriptor holds for one sector (0 = Z: the X checks measure it; 1 = X): the checks' measurements, checks, detectors, logicals.
struct SectorDesc { const int32_t *spos, *sptr; int nchk, nsyn; const uint8_t *L; };
static SectorDesc sector_desc(const qldpc_circuit_desc *D, int sector) {
    if (sector) return {D->z_syn_positions, D->z_syn_ptrs, D->num_z_checks, D->z_syn_ptrs[D->num_z_checks], D->Lz};
    return {D->x_syn_positions, D->x_syn_ptrs, D->num_x_checks, D->x_syn_ptrs[D->num_x_checks], D->Lx};
}

// Builds the per-(location, slot) signatures of one sector with the batched single-fault frame simulation.
// Every base op is an error location (kernels.py:206-351 visits them in order); the frames run through the base circuit and its suffix.
static int build_signatures(const qldpc_circuit_desc *D, int sector, std::vector<int32_t> &ptr, std::vector<uint16_t> &idx, std::vector<uint64_t> &logm) {
    std::vector<int32_t> ops(D->base_ops, D->base_ops + D->base_len), q1(D->base_q1, D->base_q1 + D->base_len), q2(D->base_q2, D->base_q2 + D->base_len);
    ops.insert(ops.end(), D->suffix_ops, D->suffix_ops + D->suffix_len);
    q1.insert(q1.end(), D->suffix_q1, D->suffix_q1 + D->suffix_len);
    q2.insert(q2.end(), D->suffix_q2, D->suffix_q2 + D->suffix_len);
    const int n_locs = (int)D->base_len, nl = 2 * n_locs, tq = D->total_qubits;
    const auto [spos, sptr, nchk, nsyn, L] = sector_desc(D, sector);
    std::vector<int32_t> lane_pos(nl), lane_q(nl);
    std::vector<int8_t> lane_after(nl);
    for (int l = 0; l < n_locs; l++) {
        const int op = D->base_ops[l];
        for (int s = 0; s < 2; s++) {
            const int e = 2 * l + s;
            lane_pos[e] = l;
            lane_after[e] = (op == C_OP_PREP_X || op == C_OP_PREP_Z || op == C_OP_CNOT) ? 1 : 0;      // Meas: before; Idle: either
            lane_q[e] = (s == 0) ? D->base_q1[l] : (op == C_OP_CNOT ? D->base_q2[l] : -1);
        }
    }
    const size_t len = ops.size();
    std::vector<int8_t> hist((size_t)nsyn * nl), state((size_t)tq * nl);
    HostStage S;
    const auto dpos = S.in(lane_pos.data(), nl);
    const auto dafter = S.in(lane_after.data(), nl);
    const auto dq = S.in(lane_q.data(), nl);
    const auto dops = S.in(ops.data(), len), dq1 = S.in(q1.data(), len), dq2 = S.in(q2.data(), len);
    const auto dstate = S.out(state.data(), tq, nl);
    const auto dhist = S.out_zeroed(hist.data(), nsyn, nl);
    int rc = S.stage();
    if (rc != QLDPC_OK) return rc;
    const unsigned grid = (unsigned)((nl + 255) / 256);
    if (sector)
        hipLaunchKernelGGL(fault_signature_kernel<true>, dim3(grid), dim3(256), 0, nullptr, nl, S[dpos], S[dafter], S[dq], (int64_t)len, S[dops], S[dq1],
                           S[dq2], tq, nsyn, S[dstate], S[dhist]);
    else
        hipLaunchKernelGGL(fault_signature_kernel<false>, dim3(grid), dim3(256), 0, nullptr, nl, S[dpos], S[dafter], S[dq], (int64_t)len, S[dops], S[dq1],
                           S[dq2], tq, nsyn, S[dstate], S[dhist]);
    QLDPC_HIP_TRY(hipGetLastError());
    if ((rc = S.finish("fault signature kernel", HostStage::kDevice)) != QLDPC_OK) return rc;
    // detectors = XOR of consecutive RAW measurements of the same check (sparsify_syndrome_jit, kernels.py:356-380)
    ptr.assign(nl + 1, 0); idx.clear(); logm.assign(nl, 0);
    std::vector<int32_t> prev(nsyn, -1);
    for (int c = 0; c < nchk; c++)
        for (int i = sptr[c] + 1; i < sptr[c + 1]; i++) prev[spos[i]] = spos[i - 1];
    for (int e = 0; e < nl; e++) {
        if (lane_q[e] >= 0)
            for (int s = 0; s < nsyn; s++) {
                int v = hist[(size_t)s * nl + e];
                if (prev[s] >= 0) v ^= hist[(size_t)prev[s] * nl + e];
                if (v & 1) idx.push_back((uint16_t)s);
            }
        ptr[e + 1] = (int32_t)idx.size();
        uint64_t lm = 0;
        if (lane_q[e] >= 0)
            for (int r = 0; r < D->k; r++) {                          // true logical = L @ data_state (simulation.py:80-81, 98-99)
                int s = 0;
                for (int j = 0; j < D->n_data; j++) s ^= (L[(size_t)r * D->n_data + j] & state[(size_t)D->data_qubit_indices[j] * nl + e] & 1);
                if (s) lm |= (uint64_t)1 << r;
            }
        logm[e] = lm;
    }
    return QLDPC_OK;
}

static int validate_desc(const qldpc_circuit_desc *D) {
    QLDPC_REQUIRE(D != nullptr, "circuit descriptor is NULL");
    QLDPC_REQUIRE(D->base_len >= 0 && D->suffix_len >= 0 && D->total_qubits > 0, "bad circuit sizes");
    QLDPC_REQUIRE(D->base_ops && D->base_q1 && D->base_q2 && (D->suffix_len == 0 || (D->suffix_ops && D->suffix_q1 && D->suffix_q2)), "NULL op array");
    QLDPC_REQUIRE(D->x_syn_positions && D->x_syn_ptrs && D->z_syn_positions && D->z_syn_ptrs && D->data_qubit_indices && D->Lx && D->Lz, "NULL table");
    QLDPC_REQUIRE(D->k >= 0 && D->k <= 64, "k out of range (0..64)");
    for (int pass = 0; pass < 2; pass++) {
        const int64_t len = pass ? D->suffix_len : D->base_len;
        const int32_t *o = pass ? D->suffix_ops : D->base_ops, *a = pass ? D->suffix_q1 : D->base_q1, *c = pass ? D->suffix_q2 : D->base_q2;
        for (int64_t i = 0; i < len; i++) {
            QLDPC_REQUIRE(o[i] >= C_OP_CNOT && o[i] <= C_OP_IDLE, "op %d at %lld is not a base-circuit gate", o[i], (long long)i);
            QLDPC_REQUIRE(a[i] >= 0 && a[i] < D->total_qubits, "q1 out of range at op %lld", (long long)i);
            QLDPC_REQUIRE(o[i] != C_OP_CNOT || (c[i] >= 0 && c[i] < D->total_qubits), "q2 out of range at op %lld", (long long)i);
        }
    }
    for (int j = 0; j < D->n_data; j++) QLDPC_REQUIRE(D->data_qubit_indices[j] >= 0 && D->data_qubit_indices[j] < D->total_qubits, "data qubit index out of range");
    return QLDPC_OK;
}

// Single-fault signatures of one sector (what the reference's builder simulates fault by fault, src/noise/builder.py:37-66).
// Entry e = 2 * base_op_index + slot (slot 0 = the gate's first qubit, slot 1 = the CNOT target).  ptr int32[2*base_len+1],
// idx uint16[idx_cap] (detector indices, ascending per entry), logmask uint64[2*base_len].  *idx_needed receives the total
// number of detector entries; QLDPC_ERR_INVALID if idx_cap is too small (call again with a larger buffer).
QLDPC_EXPORT int qldpc_circuit_fault_signatures(const qldpc_circuit_desc *D, int sector_is_x, int32_t *ptr, uint16_t *idx, int64_t idx_cap,
                                                uint64_t *logmask, int64_t *idx_needed) {
    int rc = validate_desc(D);
    if (rc != QLDPC_OK) return rc;
    QLDPC_REQUIRE(ptr && logmask && idx_needed && (idx || idx_cap == 0), "NULL output");
    QLDPC_USE_DEVICE(0);
    std::vector<int32_t> p;
    std::vector<uint16_t> ix;
    std::vector<uint64_t> lm;
    if ((rc = build_signatures(D, sector_is_x != 0, p, ix, lm)) != QLDPC_OK) return rc;
    *idx_needed = (int64_t)ix.size();
    QLDPC_REQUIRE((int64_t)ix.size() <= idx_cap, "idx buffer too small: need %lld entries", (long long)ix.size());
    std::memcpy(ptr, p.data(), p.size() * sizeof(int32_t));
    if (!ix.empty()) std::memcpy(idx, ix.data(), ix.size() * sizeof(uint16_t));
    std::memcpy(logmask, lm.data(), lm.size() * sizeof(uint64_t));
    return QLDPC_OK;
}

// One sector of a new plan: the decoder's view (graph, prior, alpha table, column logical masks), the sampler's tables (ptr / idx / log: fault
// signatures of a circuit, or the projection of a detector error model's mechanisms) and the per-trial buffers.
struct SectorIn { const qldpc_graph *g; const double *prior; const uint64_t *logmask; double alpha_val; const double *alpha_seq; int alpha_len; };
static int plan_sector(qldpc_circuit_plan *P, int i, const SectorIn &in, int alpha_mode, int layer_rows, const std::vector<int32_t> &sp,
                       const std::vector<uint16_t> &si, const std::vector<uint64_t> &sl) {
    Sector &S = P->sec[i];
    const size_t n = (size_t)in.g->n, Bz = (size_t)P->batch;
    int rc;
    S.g = in.g; S.nsyn = in.g->m; S.layer_rows = layer_rows;
    if ((rc = build_alpha_table(P->max_iter, alpha_mode, in.alpha_val, in.alpha_seq, in.alpha_len, S.h_alpha)) != QLDPC_OK) return rc;
    S.h_prior.assign(in.prior, in.prior + n);
    // "clean" inputs (finite, no -0.0 priors, positive finite clip / alphas) select the lean kernel; graphs with degree-1 checks
    // (+-inf messages) still keep the NaN test of kernels.py:328 inside it
    P->nanfree = P->nanfree && inputs_clean(in.prior, (int)n, P->clip, S.h_alpha.data(), P->max_iter);
    const std::vector<uint64_t> lm(in.logmask, in.logmask + n);
    if ((rc = upload(S.d_ptr, sp)) || (rc = upload(S.d_idx, si)) || (rc = upload(S.d_log, sl)) || (rc = upload(S.d_alpha, S.h_alpha)) || (rc = upload(S.d_prior, S.h_prior)) ||
        (rc = upload(S.d_lm, lm)) || (rc = S.d_syn.ensure(Bz * S.nsyn)) || (rc = S.d_true.ensure(Bz * 8)) || (rc = S.d_det.ensure(Bz * n)) ||
        (rc = S.d_llr.ensure(Bz * n * 8)) || (rc = S.d_conv.ensure(Bz)) || (rc = S.d_iter.ensure(Bz * 4)) || (rc = S.d_list.ensure(Bz * 4)))
        return rc;
    return QLDPC_OK;
}

// what a new plan holds once, whatever it samples: the arguments of both creation entry points, then (after the sectors) the buffers
static std::unique_ptr<qldpc_circuit_plan> plan_new(int device, int nsec, int n_locs, int max_iter, double damping, double clip_llr, int use_osd, int flags, int64_t batch) {
    std::unique_ptr<qldpc_circuit_plan> P(new qldpc_circuit_plan());
    P->device = device; P->nsec = nsec; P->n_locs = n_locs;
    P->max_iter = max_iter; P->use_osd = use_osd; P->flags = flags; P->damping = damping; P->clip = clip_llr; P->batch = batch;
    P->nanfree = true;
    return P;
}
static int plan_common(qldpc_circuit_plan *P) {
    int rc;
    if ((rc = P->d_count.ensure(64)) || (rc = P->d_tally.ensure(QLDPC_TALLY_SLOTS * 8)) || (rc = P->d_clk.ensure(2 * kClkSlots * 16))) return rc;
    if (zero_now(P->d_clk.p, 2 * kClkSlots * 16) != hipSuccess) { set_error("memset failed"); return QLDPC_ERR_HIP; }
    if (zero_now(P->d_tally.p, QLDPC_TALLY_SLOTS * 8) != hipSuccess) { set_error("memset failed"); return QLDPC_ERR_HIP; }
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_circuit_plan_create(const qldpc_circuit_desc *D, const qldpc_graph *gz, const qldpc_graph *gx, const double *prior_z,
                                           const double *prior_x, const uint64_t *logmask_z, const uint64_t *logmask_x, double p, int max_iter,
                                           int alpha_mode, double alpha_val_z, double alpha_val_x, const double *alpha_seq_z, int alpha_len_z,
                                           const double *alpha_seq_x, int alpha_len_x, double damping, double clip_llr, int use_osd, int flags,
                                           int64_t batch, qldpc_circuit_plan **out) {
    QLDPC_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    int rc = validate_desc(D);
    if (rc != QLDPC_OK) return rc;
    QLDPC_REQUIRE(gz && gx && prior_z && prior_x && logmask_z && logmask_x, "NULL argument");
    QLDPC_REQUIRE(p > 0.0 && p < 1.0, "error rate must be in (0,1)");
    QLDPC_REQUIRE(batch > 0 && batch <= (1 << 24), "batch out of range");
    QLDPC_REQUIRE(gz->device == gx->device, "both sector graphs must live on the same device");
    const SectorDesc sd[2] = {sector_desc(D, 0), sector_desc(D, 1)};
    QLDPC_REQUIRE(gz->m == sd[0].nsyn && gx->m == sd[1].nsyn, "decoding matrices have %d / %d rows but the circuit measures %d X / %d Z syndromes", gz->m,
                  gx->m, sd[0].nsyn, sd[1].nsyn);
    QLDPC_REQUIRE(sd[0].nsyn < 65536 && sd[1].nsyn < 65536, "too many detectors for 16-bit signature indices");
    QLDPC_USE_DEVICE(gz->device);
    const std::vector<uint8_t> loc_type(D->base_ops, D->base_ops + D->base_len);      // error location l = base op l

    const SectorIn in[2] = {{gz, prior_z, logmask_z, alpha_val_z, alpha_seq_z, alpha_len_z}, {gx, prior_x, logmask_x, alpha_val_x, alpha_seq_x, alpha_len_x}};
    std::unique_ptr<qldpc_circuit_plan> owner = plan_new(gz->device, 2, (int)loc_type.size(), max_iter, damping, clip_llr, use_osd, flags, batch);
    qldpc_circuit_plan *const P = owner.get();
    P->k = P->ks[0] = P->ks[1] = D->k; P->p = p; P->thr = bernoulli_threshold(p);
    for (int i = 0; i < 2; i++) {
        std::vector<int32_t> sp;
        std::vector<uint16_t> si;
        std::vector<uint64_t> sl;
        if ((rc = build_signatures(D, i, sp, si, sl)) != QLDPC_OK || (rc = plan_sector(P, i, in[i], alpha_mode, sd[i].nchk, sp, si, sl)) != QLDPC_OK) return rc;
    }
    if ((rc = upload(P->d_loc_type, loc_type)) != QLDPC_OK || (rc = plan_common(P)) != QLDPC_OK) return rc;
    *out = owner.release();
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_circuit_plan_create_dem(const qldpc_dem_desc *D, const qldpc_graph *g0, const qldpc_graph *g1, const double *prior0,
                                               const double *prior1, const uint64_t *logmask0, const uint64_t *logmask1, int max_iter, int alpha_mode,
                                               double alpha_val0, double alpha_val1, const double *alpha_seq0, int alpha_len0, const double *alpha_seq1,
                                               int alpha_len1, double damping, double clip_llr, int use_osd, int flags, int64_t batch,
                                               qldpc_circuit_plan **out) {
    QLDPC_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    int rc = dem_validate(D);
    if (rc != QLDPC_OK) return rc;
    const int nsec = D->n_sectors;
    QLDPC_REQUIRE(g0 && prior0 && logmask0, "sector 0: NULL graph, prior or logmask");
    if (nsec == 2) QLDPC_REQUIRE(g1 && prior1 && logmask1, "sector 1: NULL graph, prior or logmask");
    else QLDPC_REQUIRE(!g1 && !prior1 && !logmask1, "a detector error model with one sector takes no graph, prior or logmask of sector 1");
    QLDPC_REQUIRE(batch > 0 && batch <= (1 << 24), "batch out of range");
    QLDPC_REQUIRE(nsec == 1 || g0->device == g1->device, "both sector graphs must live on the same device");
    const SectorIn in[2] = {{g0, prior0, logmask0, alpha_val0, alpha_seq0, alpha_len0}, {g1, prior1, logmask1, alpha_val1, alpha_seq1, alpha_len1}};
    for (int i = 0; i < nsec; i++) {
        QLDPC_REQUIRE(in[i].g->m == D->n_det[i], "sector %d: the decoding matrix has %d rows but the detector error model has %d detectors", i, in[i].g->m,
                      D->n_det[i]);
        const uint64_t allowed = D->k[i] == 64 ? ~(uint64_t)0 : (((uint64_t)1 << D->k[i]) - 1);
        for (int j = 0; j < in[i].g->n; j++)
            QLDPC_REQUIRE((in[i].logmask[j] & ~allowed) == 0, "sector %d: the logical mask of column %d has a bit at or above k = %d", i, j, D->k[i]);
    }
    QLDPC_USE_DEVICE(g0->device);

    std::unique_ptr<qldpc_circuit_plan> owner = plan_new(g0->device, nsec, (int)D->n_mech, max_iter, damping, clip_llr, use_osd, flags, batch);
    qldpc_circuit_plan *const P = owner.get();
    P->dem = true; P->k = std::max(D->k[0], nsec == 2 ? D->k[1] : 0);
    const size_t nm = (size_t)D->n_mech;
    for (int i = 0; i < nsec; i++) {
        P->ks[i] = D->k[i];
        const std::vector<int32_t> sp(D->det_ptr[i], D->det_ptr[i] + nm + 1);
        const std::vector<uint16_t> si(D->det_idx[i], D->det_idx[i] + sp[nm]);
        const std::vector<uint64_t> sl(D->logmask[i], D->logmask[i] + nm);
        if ((rc = plan_sector(P, i, in[i], alpha_mode, D->layer_rows[i], sp, si, sl)) != QLDPC_OK) return rc;
    }
    std::vector<uint32_t> thr((nm + 3) / 4 * 4, 0u);                      // zero padding: a padded entry never fires
    for (size_t l = 0; l < nm; l++) {
        thr[l] = bernoulli_threshold(D->prob[l]);
        if (P->dem_odd < 0 && thr[l] != thr[0]) P->dem_odd = (int64_t)l;
    }
    if ((rc = upload(P->d_thr, thr)) != QLDPC_OK || (rc = plan_common(P)) != QLDPC_OK) return rc;
    *out = owner.release();
    return QLDPC_OK;
}

static int launch_sampler(qldpc_circuit_plan *P, uint64_t seed, int64_t begin, int64_t B, hipStream_t s, bool zero_counts = false) {
    const Sector &Z = P->sec[0], &X = P->sec[1];
    const auto sig = [](const Sector &S) { return SigTab{S.d_ptr.as<int32_t>(), S.d_idx.as<uint16_t>(), S.d_log.as<uint64_t>()}; };
    const SampleOut out{Z.nsyn, X.nsyn, P->nsec == 2, Z.d_syn.as<int8_t>(), X.d_syn.as<int8_t>(), Z.d_true.as<unsigned long long>(),
                        X.d_true.as<unsigned long long>(), zero_counts ? P->d_count.as<int32_t>() : (int32_t *)nullptr};
    switch (P->sampler) {
    case Sampler::FIXED_WEIGHT:
        return fixed_weight_sample_launch(P->device, B, begin, seed, P->fixed_weight, P->n_locs, P->dem, P->d_loc_type.as<uint8_t>(), sig(Z), sig(X), out, s);
    case Sampler::ERASURE:
        return erasure_sample_launch(P->device, B, begin, seed, P->thr, P->ethr, P->n_locs, P->d_loc_type.as<uint8_t>(), sig(Z), sig(X), out,
                                     P->d_erased.as<uint32_t>(), s);
    case Sampler::NOISE_MODEL:
        return noise_model_sample_launch(B, begin, seed, P->nm, P->n_locs, P->d_loc_cls.as<uint32_t>(), sig(Z), sig(X), out, s);
    case Sampler::SOFT:
        return soft_sample_launch(B, begin, seed, P->thr, P->sr, P->n_locs, P->d_loc_type.as<uint8_t>(), P->d_loc_cls.as<uint32_t>(),
                                  P->d_meas_rank.as<int32_t>(), P->n_meas, sig(Z), sig(X), out, P->d_levels.as<uint8_t>(), s);
    case Sampler::INDEPENDENT:
        break;
    }
    if (P->dem) return dem_sample_launch(B, begin, seed, P->n_locs, P->d_thr.as<uint32_t>(), sig(Z), sig(X), out, s);
    const SampleShape shape = sample_shape(out.n0, out.n1, true, B);
    hipLaunchKernelGGL(circuit_sample_kernel, dim3(shape.grid), dim3(256), shape.words * 4, s, B, begin, (uint32_t)seed, (uint32_t)(seed >> 32), P->thr, P->n_locs,
                       P->d_loc_type.as<uint8_t>(), sig(Z), sig(X), out);
    QLDPC_HIP_TRY(hipGetLastError());
    return QLDPC_OK;
}

// Path::ERASURE: the per-shot prior of sector `sector` from the herald record of the batch in d_erased
static int launch_erasure_prior(qldpc_circuit_plan *P, int sector, int64_t B, hipStream_t s) {
    const Sector &S = P->sec[sector];
    return erasure_prior_launch(P->device, B, P->n_locs, P->d_erased.as<uint32_t>(), S.d_er_ptr.as<int32_t>(), S.d_er_col.as<int32_t>(), S.d_er_h.as<uint8_t>(),
                                S.g->n, S.d_er_lutptr.as<int32_t>(), S.d_er_lut.as<double>(), S.d_eprior.as<double>(), s);
}

// Path::SOFT: the per-shot prior of sector `sector` from the level record of the batch in d_levels
static int launch_soft_prior(qldpc_circuit_plan *P, int sector, int64_t B, hipStream_t s) {
    const Sector &S = P->sec[sector];
    return soft_prior_launch(P->device, B, P->soft_levels, P->n_meas, P->d_levels.as<uint8_t>(), S.d_so_col.as<int32_t>(), S.d_so_w.as<int32_t>(), S.g->n,
                             S.d_so_lutptr.as<int32_t>(), S.d_so_lut.as<double>(), S.d_eprior.as<double>(), s);
}

// enqueues the decode of sector `sector` (0 = Z, 1 = X) of a batch on s, inside that sector's phase brackets.  heralds: the batch came from the
// erasure sampler (or the soft-readout sampler) and d_eprior holds its per-shot priors (Path::ERASURE and Path::SOFT read them; without, they
// decode with the plan's prior)
static int decode_sector(qldpc_circuit_plan *P, int sector, int64_t B, hipStream_t s, uint64_t seed, int64_t trial_begin, bool heralds = false) {
    Sector &S = P->sec[sector];
    const qldpc_graph *g = S.g;
    int rc = QLDPC_OK;
    int32_t *count = P->fail_count(sector);
    const int ph_bp = kPhaseBp[sector], ph_osd = kPhaseOsd[sector];
    unsigned long long *clk = (P->flags & QLDPC_FLAG_CLOCK_PROBE) ? P->d_clk.as<unsigned long long>() : nullptr;
    if (P->path != Path::WINDOW && (rc = phase_mark(P, ph_bp, s, true)) != QLDPC_OK) return rc;      // (the window loop marks its own brackets)
    switch (P->path) {
    case Path::WINDOW: {  // the window loop in the two brackets: BP = gather + min-sum, OSD = collect + OSD-0 + commit, summed over the windows
        const WindowPlanSlots slots{S.d_conv.as<uint8_t>(), S.d_iter.as<int32_t>(), count};
        const std::function<int(int, bool)> mark = [&](int part, bool open) { return phase_mark(P, part ? ph_osd : ph_bp, s, open); };
        return window_decoder_lock_and_launch(S.win.get(), B, S.d_syn.as<int8_t>(), S.d_det.as<int8_t>(), &slots, &mark, s);
    }
    case Path::RELAY: {   // Relay-BP in the BP phase's bracket; no OSD stage (its phase time stays 0)
        std::lock_guard<std::mutex> lk(g->mu);
        // iter_bias -1: the judge adds one per trial, so the ITERS slots sum the Relay-BP iterations
        rc = relay_decode_launch(g, B, S.d_syn.as<int8_t>(), S.d_prior.as<double>(), P->rp, seed, trial_begin, sector, -1, S.d_det.as<int8_t>(),
                                 S.d_conv.as<uint8_t>(), S.d_legs.as<int32_t>(), S.d_iter.as<int32_t>(), nullptr, s);
        break;
    }
    case Path::LAYERED:   // the layered schedule: same outputs, so the OSD stage below takes them unchanged
        rc = layered_lock_and_launch(S.lay.get(), B, S.d_syn.as<int8_t>(), S.d_det.as<int8_t>(), S.d_llr.as<double>(), S.d_conv.as<uint8_t>(), S.d_iter.as<int32_t>(), s);
        break;
    case Path::F32:       // single precision: same outputs (the posteriors widened to f64)
        rc = minsum32_lock_and_launch(S.f32.get(), B, S.d_syn.as<int8_t>(), S.d_det.as<int8_t>(), S.d_llr.as<double>(), S.d_conv.as<uint8_t>(), S.d_iter.as<int32_t>(), s);
        break;
    case Path::DECIM: {   // guided decimation: same outputs too; iter_bias -1 as for Relay-BP, the rounds go where its legs go
        std::lock_guard<std::mutex> lk(g->mu);
        rc = decim_decode_launch(g, B, S.d_syn.as<int8_t>(), S.d_prior.as<double>(), P->dp, -1, S.d_det.as<int8_t>(), S.d_llr.as<double>(),
                                 S.d_conv.as<uint8_t>(), S.d_iter.as<int32_t>(), S.d_legs.as<int32_t>(), nullptr, s);
        break;
    }
    case Path::CORRELATED: {   // the per-shot-prior kernel: sector 0 as it is; sector 1 with the links, read against sector 0's correction as its OSD stage left it
        const Sector &Z = P->sec[0];
        const ShotLinks none{0, nullptr, nullptr, nullptr, nullptr};
        const ShotLinks links{Z.g->n, Z.d_det.as<int8_t>(), P->d_cl_ptr.as<int32_t>(), P->d_cl_src.as<int32_t>(), P->d_cl_llr.as<double>()};
        const double *prior = sector == 1 && P->corr_base ? P->d_cl_base.as<double>() : S.d_prior.as<double>();
        std::lock_guard<std::mutex> lk(g->mu);
        rc = shotprior_decode_launch(g, B, S.d_syn.as<int8_t>(), prior, 0, sector == 1 ? links : none, P->corr_alpha, P->clip, P->max_iter, -1,
                                     S.d_det.as<int8_t>(), S.d_llr.as<double>(), S.d_conv.as<uint8_t>(), S.d_iter.as<int32_t>(), nullptr, s);
        break;
    }
    case Path::ERASURE:        // the per-shot-prior kernel with no links: prior[B][n] of the batch's heralds, or the plan's prior where there are none
    case Path::SOFT: {         // ... and the same launch for the batch's readout levels
        const ShotLinks none{0, nullptr, nullptr, nullptr, nullptr};
        std::lock_guard<std::mutex> lk(g->mu);
        rc = shotprior_decode_launch(g, B, S.d_syn.as<int8_t>(), heralds ? S.d_eprior.as<double>() : S.d_prior.as<double>(), heralds ? g->n : 0, none,
                                     P->path == Path::SOFT ? P->soft_alpha : P->era_alpha, P->clip, P->max_iter, -1, S.d_det.as<int8_t>(), S.d_llr.as<double>(), S.d_conv.as<uint8_t>(),
                                     S.d_iter.as<int32_t>(), nullptr, s);
        break;
    }
    case Path::FLOOD: {
        std::lock_guard<std::mutex> lk(g->mu);
        g->clk_probe = (clk && sector == 0) ? clk : nullptr;                  // sector Z carries the probe (one writer per buffer)
        rc = minsum_decode_dispatch(g, B, S.d_syn.as<int8_t>(), S.d_prior.as<double>(), P->max_iter, S.d_alpha.as<double>(), P->damping, P->clip,
                                    (P->flags & QLDPC_FLAG_PUBLIC_MASK) | (P->nanfree ? QLDPC_FLAG_INTERNAL_PRIOR_FINITE : 0), P->nanfree,
                                    S.d_det.as<int8_t>(), S.d_llr.as<double>(), S.d_conv.as<uint8_t>(), S.d_iter.as<int32_t>(), s,
                                    S.h_prior.empty() ? nullptr : S.h_prior.data());
        g->clk_probe = nullptr;
        break;
    }
    }
    if (rc != QLDPC_OK) return rc;
    if ((rc = phase_mark(P, ph_bp, s, false)) != QLDPC_OK || !P->osd_stage()) return rc;
    if ((rc = phase_mark(P, ph_osd, s, true)) != QLDPC_OK) return rc;
    hipLaunchKernelGGL(collect_failed2_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, B, S.d_conv.as<uint8_t>(), S.d_list.as<int32_t>(), count);
    {
        std::lock_guard<std::mutex> lk(g->mu);
        g->clk_probe = (clk && sector == 0) ? clk + 2 * kClkSlots : nullptr;
        if (P->osd == Osd::CS)
            rc = osdcs_listed_launch(g, S.d_list.as<int32_t>(), count, B, S.d_syn.as<int8_t>(), S.d_llr.as<double>(), S.d_det.as<int8_t>(),
                                     S.d_prior.as<double>(), P->cs_order, S.d_det.as<int8_t>(), S.d_flips.as<int32_t>(), s);
        else if (P->osd == Osd::LSD) {
            const bool conf = P->conf_kind >= 0;                              // a converged shot has nothing to solve: its row stays zero
            if (conf && hipMemsetAsync(S.d_lsd_stats.p, 0, (size_t)B * 64, s) != hipSuccess) { set_error("hipMemsetAsync failed"); rc = QLDPC_ERR_HIP; }
            if (rc == QLDPC_OK)
                rc = lsd_listed_launch(g, S.d_list.as<int32_t>(), count, B, S.d_syn.as<int8_t>(), S.d_llr.as<double>(), S.d_det.as<int8_t>(), P->lsd_bits,
                                       P->lsd_rows, S.d_det.as<int8_t>(), S.d_lsd_info.as<int32_t>(), P->d_lsd_counts.as<unsigned long long>() + 3 * sector,
                                       conf && S.has_conf_w ? S.d_conf_w.as<uint16_t>() : nullptr, conf ? S.d_lsd_stats.as<unsigned long long>() : nullptr, s);
        }
        else
            rc = osd0_listed_launch(g, S.d_list.as<int32_t>(), count, B, S.d_syn.as<int8_t>(), S.d_llr.as<double>(), S.d_det.as<int8_t>(), nullptr,
                                    S.d_det.as<int8_t>(), P->flags, s);
        g->clk_probe = nullptr;
    }
    if (rc != QLDPC_OK) return rc;
    QLDPC_HIP_TRY(hipGetLastError());
    return phase_mark(P, ph_osd, s, false);                      // (the judge kernel adds the two failure counts to the OSD tally slots)
}

static JudgeSector judge_view(const Sector &S) {
    const qldpc_graph *g = S.g;
    return {g->m, g->n, g->d_indptr, g->d_indices, g->d_colptr, g->d_rowidx, S.d_lm.as<uint64_t>(), S.d_syn.as<int8_t>(), S.d_det.as<int8_t>(),
            S.d_conv.as<uint8_t>(), S.d_iter.as<int32_t>(), S.d_true.as<unsigned long long>()};
}

// the score kernel on the batch in flight (qldpc_circuit_plan_use_confidence): d_score from the sectors' statistics, and with d_outcome the histogram
static int launch_confidence(qldpc_circuit_plan *P, int64_t B, const uint8_t *d_outcome, hipStream_t s) {
    return confidence_launch(P->device, B, P->conf_kind, P->sec[0].d_lsd_stats.as<unsigned long long>(),
                             P->nsec == 2 ? P->sec[1].d_lsd_stats.as<unsigned long long>() : nullptr, d_outcome, P->d_score.as<unsigned long long>(),
                             d_outcome ? P->conf_bins : 1, P->d_edges.as<unsigned long long>(), d_outcome ? P->d_hist.as<unsigned long long>() : nullptr, s);
}

// one pass over [trial_begin, trial_begin + count); `outcome` (host, may be NULL) receives bit0 = z_err, bit1 = x_err per trial, `score` (host, may be
// NULL; a plan with a confidence only) the trial's score.  A plan with a confidence writes the outcome byte of every batch: its histogram reads it.
static int circuit_run(qldpc_circuit_plan *P, uint64_t seed, int64_t trial_begin, int64_t count, hipStream_t s, uint8_t *outcome, uint64_t *score = nullptr) {
    QLDPC_USE_DEVICE(P->device);
    int rc;
    const bool conf = P->conf_kind >= 0, bytes = outcome || conf;
    if (bytes && (rc = P->d_outcome.ensure((size_t)P->batch)) != QLDPC_OK) return rc;
    const bool two = P->nsec == 2;
    const JudgeSector Z = judge_view(P->sec[0]), X = two ? judge_view(P->sec[1]) : JudgeSector{};
    const bool sparse = Z.m <= 4096 && Z.colptr && (!two || (X.m <= 4096 && X.colptr));
    const auto judge = two ? (sparse ? circuit_judge_kernel<true, true> : circuit_judge_kernel<false, true>)
                           : (sparse ? circuit_judge_kernel<true, false> : circuit_judge_kernel<false, false>);
    for (int64_t off = 0; off < count; off += P->batch) {
        const int64_t B = std::min<int64_t>(P->batch, count - off);
        if (P->pending.size() > 256) drain_phases(P, false);         // a caller that never reads phase times: recycle finished brackets (bounded event count)
        if ((rc = phase_mark(P, QLDPC_PHASE_SAMPLE, s, true)) != QLDPC_OK) return rc;
        if ((rc = launch_sampler(P, seed, trial_begin + off, B, s, true)) != QLDPC_OK) return rc;
        const bool levels = P->sampler == Sampler::SOFT && P->path == Path::SOFT;
        const bool heralds = (P->sampler == Sampler::ERASURE && P->path == Path::ERASURE) || levels;       // (the prior kernels count as sampling: they turn the draws into the decoder's input)
        for (int sector = 0; heralds && sector < P->nsec; sector++)
            if ((rc = levels ? launch_soft_prior(P, sector, B, s) : launch_erasure_prior(P, sector, B, s)) != QLDPC_OK) return rc;
        if ((rc = phase_mark(P, QLDPC_PHASE_SAMPLE, s, false)) != QLDPC_OK) return rc;
        for (int sector = 0; sector < P->nsec; sector++)
            if ((rc = decode_sector(P, sector, B, s, seed, trial_begin + off, heralds)) != QLDPC_OK) return rc;
        if ((rc = phase_mark(P, QLDPC_PHASE_JUDGE, s, true)) != QLDPC_OK) return rc;
        hipLaunchKernelGGL(judge, dim3((unsigned)((B + 7) / 8)), dim3(256), 0, s, B, Z, X, P->d_tally.as<unsigned long long>(),
                           bytes ? P->d_outcome.as<uint8_t>() : (uint8_t *)nullptr, P->osd_stage() ? P->d_count.as<int32_t>() : (const int32_t *)nullptr);
        QLDPC_HIP_TRY(hipGetLastError());
        if (conf && (rc = launch_confidence(P, B, P->d_outcome.as<uint8_t>(), s)) != QLDPC_OK) return rc;
        if ((P->path == Path::RELAY || P->path == Path::DECIM) &&
            (rc = relay_legs_tally_launch(B, P->sec[0].d_legs.as<int32_t>(), two ? P->sec[1].d_legs.as<int32_t>() : nullptr, P->d_tally.as<unsigned long long>(), s)) != QLDPC_OK)
            return rc;
        if ((rc = phase_mark(P, QLDPC_PHASE_JUDGE, s, false)) != QLDPC_OK) return rc;
        P->batches++;
        if (outcome) {
            QLDPC_HIP_TRY(hipMemcpyAsync(outcome + off, P->d_outcome.p, (size_t)B, hipMemcpyDeviceToHost, s));
            if (score) QLDPC_HIP_TRY(hipMemcpyAsync(score + off, P->d_score.p, (size_t)B * 8, hipMemcpyDeviceToHost, s));
            QLDPC_HIP_TRY(hipStreamSynchronize(s));
        }
    }
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_circuit_plan_run(qldpc_circuit_plan *P, uint64_t seed, int64_t trial_begin, int64_t count, void *stream) {
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    QLDPC_REQUIRE(count >= 0 && trial_begin >= 0, "negative trial range");
    return circuit_run(P, seed, trial_begin, count, reinterpret_cast<hipStream_t>(stream), nullptr);
}

QLDPC_EXPORT int qldpc_circuit_plan_run_outcomes(qldpc_circuit_plan *P, uint64_t seed, int64_t trial_begin, int64_t count, void *stream,
                                                 uint8_t *outcome) {
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    QLDPC_REQUIRE(count >= 0 && trial_begin >= 0, "negative trial range");
    QLDPC_REQUIRE(count == 0 || outcome != nullptr, "outcome is NULL");
    return circuit_run(P, seed, trial_begin, count, reinterpret_cast<hipStream_t>(stream), outcome);
}

QLDPC_EXPORT int qldpc_circuit_plan_run_scores(qldpc_circuit_plan *P, uint64_t seed, int64_t trial_begin, int64_t count, void *stream, uint8_t *outcome,
                                               uint64_t *score) {
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    QLDPC_REQUIRE(count >= 0 && trial_begin >= 0, "negative trial range");
    QLDPC_REQUIRE(P->conf_kind >= 0, "the plan has no confidence (qldpc_circuit_plan_use_confidence)");
    QLDPC_REQUIRE(count == 0 || (outcome != nullptr && score != nullptr), "outcome or score is NULL");
    return circuit_run(P, seed, trial_begin, count, reinterpret_cast<hipStream_t>(stream), outcome, score);
}

QLDPC_EXPORT int qldpc_circuit_plan_read(qldpc_circuit_plan *P, void *stream, int clear, int64_t *tally) {
    QLDPC_REQUIRE(P != nullptr && tally != nullptr, "NULL argument");
    QLDPC_USE_DEVICE(P->device);
    QLDPC_HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    drain_phases(P, true);                                           // everything enqueued has finished: fold the brackets, recycle their events
    QLDPC_HIP_TRY(hipMemcpy(tally, P->d_tally.p, QLDPC_TALLY_SLOTS * 8, hipMemcpyDeviceToHost));
    if (clear) QLDPC_HIP_TRY(zero_now(P->d_tally.p, QLDPC_TALLY_SLOTS * 8));
    return QLDPC_OK;
}

// The batch loop of the three sample exports, everything to host pointers: per batch the sampler and, where priors are asked for, every sector's prior
// kernel; a wait; then per sector in use the syndromes int8[count][nsyn], the truth bits unpacked to int8[count][k] and the priors f64[count][n] out of
// d_eprior, and the batch's rows of the record.  A one-sector plan touches nothing of sector 1.
// SampleRecord: what a sampler writes per trial besides the syndromes (the herald words, the levels): `bytes` per trial from dev to host; zero: the
// plan is not on that sampler, which then writes no record, so it reads as zeros.
struct SampleRecord { void *dev; size_t bytes; void *host; bool zero; };
using PriorLaunch = int (*)(qldpc_circuit_plan *, int, int64_t, hipStream_t);
static int sample_readback(qldpc_circuit_plan *P, uint64_t seed, int64_t trial_begin, int64_t count, int8_t *const sparse[2], int8_t *const truth[2],
                           const SampleRecord &rec = {}, PriorLaunch launch_prior = nullptr, double *const prior[2] = nullptr) {
    int rc;
    std::vector<unsigned long long> t;
    for (int64_t off = 0; off < count; off += P->batch) {
        const int64_t B = std::min<int64_t>(P->batch, count - off);
        if (rec.zero && rec.bytes) QLDPC_HIP_TRY(hipMemsetAsync(rec.dev, 0, (size_t)B * rec.bytes, nullptr));
        if ((rc = launch_sampler(P, seed, trial_begin + off, B, nullptr)) != QLDPC_OK) return rc;
        for (int i = 0; launch_prior && i < P->nsec; i++)
            if ((rc = launch_prior(P, i, B, nullptr)) != QLDPC_OK) return rc;
        QLDPC_HIP_TRY(hipDeviceSynchronize());
        t.resize(B);
        if (rec.bytes) QLDPC_HIP_TRY(hipMemcpy(static_cast<uint8_t *>(rec.host) + off * rec.bytes, rec.dev, (size_t)B * rec.bytes, hipMemcpyDeviceToHost));
        for (int i = 0; i < P->nsec; i++) {
            const Sector &S = P->sec[i];
            QLDPC_HIP_TRY(hipMemcpy(sparse[i] + off * S.nsyn, S.d_syn.p, (size_t)B * S.nsyn, hipMemcpyDeviceToHost));
            QLDPC_HIP_TRY(hipMemcpy(t.data(), S.d_true.p, (size_t)B * 8, hipMemcpyDeviceToHost));
            for (int64_t b = 0; b < B; b++)
                for (int r = 0; r < P->ks[i]; r++) truth[i][(off + b) * P->ks[i] + r] = (int8_t)((t[b] >> r) & 1);
            if (launch_prior) QLDPC_HIP_TRY(hipMemcpy(prior[i] + off * S.g->n, S.d_eprior.p, (size_t)B * S.g->n * 8, hipMemcpyDeviceToHost));
        }
    }
    return QLDPC_OK;
}

// batched run_trial_fast: sparse_z int8[count][nsx], true_z int8[count][k], sparse_x int8[count][nsz], true_x int8[count][k] (host)
QLDPC_EXPORT int qldpc_circuit_plan_sample(qldpc_circuit_plan *P, uint64_t seed, int64_t trial_begin, int64_t count, int8_t *sparse_z,
                                           int8_t *true_z, int8_t *sparse_x, int8_t *true_x) {
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    QLDPC_REQUIRE(count >= 0 && trial_begin >= 0, "negative trial range");
    QLDPC_REQUIRE(count == 0 || (sparse_z && true_z && (P->nsec == 1 || (sparse_x && true_x))), "NULL output");
    QLDPC_USE_DEVICE(P->device);
    int8_t *const sparse[2] = {sparse_z, sparse_x}, *const truth[2] = {true_z, true_x};
    return sample_readback(P, seed, trial_begin, count, sparse, truth);
}

// Sums (ms) of the hipEvent brackets of each phase over the batches enqueued since the last call, and the number of batches.  The phases of
// a batch run back to back on the caller's stream, so the brackets do not overlap.
QLDPC_EXPORT int qldpc_circuit_plan_phase_times(qldpc_circuit_plan *P, double *ms, int64_t *batches) {
    QLDPC_REQUIRE(P != nullptr && ms != nullptr, "NULL argument");
    QLDPC_USE_DEVICE(P->device);
    drain_phases(P, true);
    for (int i = 0; i < QLDPC_CIRCUIT_PHASES; i++) { ms[i] = P->phase_ms[i]; P->phase_ms[i] = 0; }
    if (batches) *batches = P->batches;
    P->batches = 0;
    return QLDPC_OK;
}

// Shader clock (MHz) held while the decode kernel [0] and the OSD-0 kernel [1] of sector Z ran in the last batch: median over workgroups of
// delta(s_memtime) / delta(s_memrealtime) x 100 MHz.  Needs QLDPC_FLAG_CLOCK_PROBE at plan creation; 0 where nothing was stamped.
QLDPC_EXPORT int qldpc_circuit_plan_clock(qldpc_circuit_plan *P, void *stream, double *mhz) {
    QLDPC_REQUIRE(P != nullptr && mhz != nullptr, "NULL argument");
    QLDPC_REQUIRE(P->flags & QLDPC_FLAG_CLOCK_PROBE, "the plan was created without QLDPC_FLAG_CLOCK_PROBE");
    QLDPC_USE_DEVICE(P->device);
    QLDPC_HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    std::vector<unsigned long long> h(4 * kClkSlots);
    QLDPC_HIP_TRY(hipMemcpy(h.data(), P->d_clk.p, h.size() * 8, hipMemcpyDeviceToHost));
    for (int k = 0; k < 2; k++) mhz[k] = clock_probe_median(h.data() + 2 * kClkSlots * k, kClkSlots);
    return QLDPC_OK;
}

// The switch rules, once.  A plan decodes on two axes, and qldpc_circuit_plan_use_* moves it along one of them:
//   Path: who fills the BP bracket and its follow-up -- flooding min-sum (as created), the layered schedule, guided decimation, single precision (f32),
//     Relay-BP, sliding windows, correlated two-sector decoding, erasure-aware or soft-aware decoding.  A plan leaves flooding at most once.  Asking again for the
//     path it is on brings new arguments (Relay-BP, layered, decimation, correlated, erasure-aware, soft-aware), changes nothing (f32) or is refused (windows).
//   OSD stage: OSD-0 (as created; none with use_osd = 0), OSD-CS or LSD.  OSD-CS and LSD need use_osd, go with flooding, layered, decimation, f32,
//     correlated, erasure-aware and soft-aware whichever came first, and may be asked for again with new arguments.  They go with neither Relay-BP nor windows, whichever came first, and they
//     refuse each other in either order.
//   Confidence (qldpc_circuit_plan_use_confidence) is no axis of its own: it rides on the LSD stage, so it is legal once the OSD stage is LSD, before or
//     after the path switches that LSD goes with, and again with new arguments; everything that refuses LSD thereby refuses it.
//   Windows need use_osd as well; Relay-BP, layered, decimation, f32, correlated, erasure-aware and soft-aware do not.  Windows, layered,
//   decimation, f32, correlated, erasure-aware and soft-aware need damping = 1.
// Each switch then checks its own arguments and what its kernels need (Relay-BP, OSD-CS, decimation, correlated: finite priors and a supported graph;
// correlated: two sectors; erasure-aware and soft-aware: what correlated's kernel needs, and a circuit plan).
// `to`: the path asked for; Path::FLOOD stands for a request on the other axis, for the OSD stage `stage` (no call asks for flooding).
// QLDPC_OK, or QLDPC_ERR_INVALID with the error text set.
static int switch_allowed(const qldpc_circuit_plan *P, Path to, Osd stage = Osd::CS) {
    static const char *const path_name[] = {"BP + OSD-0", "the layered schedule", "guided decimation", "single precision (f32)", "Relay-BP", "sliding-window decoding", "correlated decoding",
                                             "erasure-aware decoding", "soft-aware decoding"};
    static const char *const osd_name[] = {"BP + OSD-0", "BP + OSD-CS", "BP + LSD"};
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    const bool cs = to == Path::FLOOD;                                   // a request on the OSD axis: `stage` says for which of the two
    const bool switched = P->osd != Osd::OSD0, other = cs && switched && P->osd != stage;      // OSD-CS and LSD refuse each other
    const auto without_cs = [](Path p) { return p == Path::RELAY || p == Path::WINDOW; };
    const char *now = other || (P->path == Path::FLOOD && switched) ? osd_name[(int)P->osd] : path_name[(int)P->path];
    const char *asked = cs ? osd_name[(int)stage] : path_name[(int)to];
    const bool follows = cs ? !without_cs(P->path) && !other : P->path == Path::FLOOD ? !(switched && without_cs(to)) : (P->path == to && to != Path::WINDOW);
    QLDPC_REQUIRE(follows, "the plan was switched to %s: %s cannot follow", now, asked);
    QLDPC_REQUIRE(P->use_osd || !(cs || to == Path::WINDOW), "the plan was created with use_osd = 0: %s needs its OSD stage", asked);
    QLDPC_REQUIRE(P->damping == 1.0 || cs || to == Path::RELAY, "%s needs damping = 1 (the plan has %g)", asked, P->damping);
    return QLDPC_OK;
}

// What Relay-BP, OSD-CS and decimation check after their own arguments (params_rc): finite priors, then a graph their kernels support in every sector.
template <class F>
static int inputs_supported(const qldpc_circuit_plan *P, int params_rc, F graph_rc) {
    if (params_rc != QLDPC_OK) return params_rc;
    for (int i = 0; i < P->nsec; i++)
        for (double v : P->sec[i].h_prior) QLDPC_REQUIRE(std::isfinite(v), "the plan's sector-%c prior is not finite", "ZX"[i]);
    for (int i = 0; i < P->nsec; i++)
        if (const int rc = graph_rc(P->sec[i].g); rc != QLDPC_OK) return rc;
    return QLDPC_OK;
}

// `bytes` in one buffer of every sector in use
static int ensure_each(qldpc_circuit_plan *P, DevBuf Sector::*buf, size_t bytes) {
    QLDPC_USE_DEVICE(P->device);
    for (int i = 0; i < P->nsec; i++)
        if (const int rc = (P->sec[i].*buf).ensure(bytes); rc != QLDPC_OK) return rc;
    return QLDPC_OK;
}

// One handle per sector in use, all or none: create(S, i, &h) builds sector i's; if one fails, what was built is destroyed and the plan keeps what it
// had.  Then every sector's `slot` takes its new handle and the one it held (if any) is destroyed.
template <class Ptr, class Create>
static int build_handles(qldpc_circuit_plan *P, Ptr Sector::*slot, Create create) {
    QLDPC_USE_DEVICE(P->device);
    Ptr h[2];
    for (int i = 0; i < P->nsec; i++) {
        typename Ptr::pointer raw = nullptr;
        if (const int rc = create(P->sec[i], i, &raw); rc != QLDPC_OK) return rc;
        h[i].reset(raw);
    }
    for (int i = 0; i < P->nsec; i++) P->sec[i].*slot = std::move(h[i]);
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_circuit_plan_use_relay(qldpc_circuit_plan *P, double alpha, double gamma0, double gamma_min, double gamma_max, int t0, int tr,
                                             int max_legs, int stop_after) {
    int rc = switch_allowed(P, Path::RELAY);
    if (rc != QLDPC_OK) return rc;
    const RelayParams rp{alpha, P->clip, gamma0, gamma_min, gamma_max, t0, tr, max_legs, stop_after};
    if ((rc = inputs_supported(P, relay_check_params(rp), [](const qldpc_graph *g) { return relay_mode(g) ? QLDPC_OK : relay_unsupported(g); })) != QLDPC_OK ||
        (rc = ensure_each(P, &Sector::d_legs, (size_t)P->batch * 4)) != QLDPC_OK)
        return rc;
    P->rp = rp;
    P->path = Path::RELAY;
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_circuit_plan_use_osd_cs(qldpc_circuit_plan *P, int order) {
    int rc = switch_allowed(P, Path::FLOOD);
    if (rc != QLDPC_OK) return rc;
    if ((rc = inputs_supported(P, osdcs_check_order(order), osdcs_supported)) != QLDPC_OK ||
        (rc = ensure_each(P, &Sector::d_flips, (size_t)P->batch * 8)) != QLDPC_OK)
        return rc;
    P->cs_order = order;
    P->osd = Osd::CS;
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_circuit_plan_use_lsd(qldpc_circuit_plan *P, int bits_per_step, int max_rows) {
    int rc = switch_allowed(P, Path::FLOOD, Osd::LSD);
    if (rc != QLDPC_OK || (rc = lsd_check_params(bits_per_step, max_rows)) != QLDPC_OK) return rc;
    for (int i = 0; i < P->nsec; i++)
        if ((rc = lsd_graph_supported(P->sec[i].g, max_rows)) != QLDPC_OK) return rc;
    if ((rc = ensure_each(P, &Sector::d_lsd_info, (size_t)P->batch * 16)) != QLDPC_OK) return rc;
    if (!P->d_lsd_counts.p) {                                            // (asked again: the counts go on)
        QLDPC_USE_DEVICE(P->device);
        if ((rc = P->d_lsd_counts.ensure(6 * 8)) != QLDPC_OK) return rc;
        QLDPC_HIP_TRY(zero_now(P->d_lsd_counts.p, 6 * 8));
    }
    P->lsd_bits = bits_per_step; P->lsd_rows = max_rows;
    P->osd = Osd::LSD;
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_circuit_plan_use_confidence(qldpc_circuit_plan *P, int kind, int nbins, const uint64_t *edges, const uint16_t *weight_z,
                                                  const uint16_t *weight_x) {
    static const char *const osd_name[] = {"BP + OSD-0", "BP + OSD-CS", "BP + LSD"};
    static const char *const path_name[] = {"", "", "", "", "Relay-BP", "sliding-window decoding", "", "", ""};
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    QLDPC_REQUIRE(P->use_osd, "the plan was created with use_osd = 0: a confidence needs its OSD stage switched to BP + LSD");
    QLDPC_REQUIRE(P->path != Path::RELAY && P->path != Path::WINDOW, "the plan was switched to %s: a confidence cannot follow (it needs BP + LSD)",
                  path_name[(int)P->path]);
    QLDPC_REQUIRE(P->osd == Osd::LSD, "the plan's OSD stage is %s: a confidence needs BP + LSD (qldpc_circuit_plan_use_lsd first)", osd_name[(int)P->osd]);
    int rc = confidence_check(kind, nbins, edges);
    if (rc != QLDPC_OK) return rc;
    const uint16_t *const weight[2] = {weight_z, weight_x};
    for (int i = 0; i < P->nsec; i++)
        QLDPC_REQUIRE(weight[i] != nullptr || kind <= QLDPC_CONF_COLS_INF, "weight_%c is NULL: only the QLDPC_CONF_COLS_* kinds go without weights", "zx"[i]);
    QLDPC_USE_DEVICE(P->device);
    QLDPC_HIP_TRY(hipDeviceSynchronize());                              // a run that is still enqueued reads the tables replaced here
    if ((rc = ensure_each(P, &Sector::d_lsd_stats, (size_t)P->batch * 64)) != QLDPC_OK || (rc = P->d_score.ensure((size_t)P->batch * 8)) != QLDPC_OK ||
        (rc = P->d_outcome.ensure((size_t)P->batch)) != QLDPC_OK || (rc = P->d_hist.ensure((size_t)nbins * 32)) != QLDPC_OK ||
        (rc = P->d_edges.ensure((size_t)std::max(nbins - 1, 1) * 8)) != QLDPC_OK)
        return rc;
    if (nbins > 1) QLDPC_HIP_TRY(hipMemcpy(P->d_edges.p, edges, (size_t)(nbins - 1) * 8, hipMemcpyHostToDevice));
    for (int i = 0; i < P->nsec; i++) {
        Sector &S = P->sec[i];
        S.has_conf_w = weight[i] != nullptr;
        if (!S.has_conf_w) continue;
        if ((rc = S.d_conf_w.ensure((size_t)std::max(S.g->n, 1) * 2)) != QLDPC_OK) return rc;
        QLDPC_HIP_TRY(hipMemcpy(S.d_conf_w.p, weight[i], (size_t)S.g->n * 2, hipMemcpyHostToDevice));
    }
    QLDPC_HIP_TRY(zero_now(P->d_hist.p, (size_t)nbins * 32));
    P->conf_kind = kind; P->conf_bins = nbins;
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_circuit_plan_confidence_read(qldpc_circuit_plan *P, void *stream, int clear, uint64_t *hist) {
    QLDPC_REQUIRE(P != nullptr && hist != nullptr, "NULL argument");
    QLDPC_REQUIRE(P->conf_kind >= 0, "the plan has no confidence (qldpc_circuit_plan_use_confidence)");
    QLDPC_USE_DEVICE(P->device);
    QLDPC_HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    QLDPC_HIP_TRY(hipMemcpy(hist, P->d_hist.p, (size_t)P->conf_bins * 32, hipMemcpyDeviceToHost));
    if (clear) QLDPC_HIP_TRY(zero_now(P->d_hist.p, (size_t)P->conf_bins * 32));
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_circuit_plan_lsd_counts(qldpc_circuit_plan *P, void *stream, int clear, int64_t *counts) {
    QLDPC_REQUIRE(P != nullptr && counts != nullptr, "NULL argument");
    QLDPC_USE_DEVICE(P->device);
    QLDPC_HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    for (int i = 0; i < 6; i++) counts[i] = 0;
    if (!P->d_lsd_counts.p) return QLDPC_OK;
    QLDPC_HIP_TRY(hipMemcpy(counts, P->d_lsd_counts.p, 6 * 8, hipMemcpyDeviceToHost));
    if (clear) QLDPC_HIP_TRY(zero_now(P->d_lsd_counts.p, 6 * 8));
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_circuit_plan_use_window(qldpc_circuit_plan *P, int window, int commit) {
    int rc = switch_allowed(P, Path::WINDOW);
    if (rc != QLDPC_OK) return rc;
    for (int i = 0; P->dem && i < P->nsec; i++)
        QLDPC_REQUIRE(P->sec[i].layer_rows > 0 && P->sec[i].nsyn % P->sec[i].layer_rows == 0,
                      "sector %d of the detector error model has layer_rows = %d, which %s: sliding-window decoding needs the rows of a syndrome cycle", i,
                      P->sec[i].layer_rows, P->sec[i].layer_rows > 0 ? "does not divide its detectors" : "means no layers were given");
    rc = build_handles(P, &Sector::win, [&](const Sector &S, int, qldpc_window_decoder **out) {
        return window_decoder_create_tab(S.g, S.layer_rows, window, commit, S.h_prior.data(), P->max_iter, S.h_alpha, P->clip, P->flags & QLDPC_FLAG_PUBLIC_MASK, out);
    });
    if (rc == QLDPC_OK) P->path = Path::WINDOW;
    return rc;
}

QLDPC_EXPORT int qldpc_circuit_plan_use_layered(qldpc_circuit_plan *P, const int32_t *row_layer_z, const int32_t *row_layer_x) {
    int rc = switch_allowed(P, Path::LAYERED);
    if (rc != QLDPC_OK) return rc;
    const int32_t *const row_layer[2] = {row_layer_z, row_layer_x};
    rc = build_handles(P, &Sector::lay, [&](const Sector &S, int i, qldpc_layered_decoder **out) {
        return layered_decoder_create_tab(S.g, row_layer[i], S.h_prior.data(), P->max_iter, S.h_alpha, P->clip, P->flags & QLDPC_FLAG_PUBLIC_MASK, out);
    });
    if (rc == QLDPC_OK) P->path = Path::LAYERED;
    return rc;
}

QLDPC_EXPORT int qldpc_circuit_plan_use_decimation(qldpc_circuit_plan *P, double alpha, int t_round, int max_rounds, int per_round, double fix_llr) {
    int rc = switch_allowed(P, Path::DECIM);
    if (rc != QLDPC_OK) return rc;
    const DecimParams dp{alpha, P->clip, fix_llr, t_round, max_rounds, per_round};
    if ((rc = inputs_supported(P, decim_check_params(dp), [](const qldpc_graph *g) { return decim_supported(g) ? QLDPC_OK : decim_unsupported(g); })) != QLDPC_OK ||
        (rc = ensure_each(P, &Sector::d_legs, (size_t)P->batch * 4)) != QLDPC_OK)
        return rc;
    P->dp = dp;
    P->path = Path::DECIM;
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_circuit_plan_use_correlated(qldpc_circuit_plan *P, double alpha, const double *base_x, int64_t n_links, const int32_t *link_ptr,
                                                   const int32_t *link_src, const double *link_llr) {
    int rc = switch_allowed(P, Path::CORRELATED);
    if (rc != QLDPC_OK) return rc;
    QLDPC_REQUIRE(P->nsec == 2, "correlated decoding needs a plan with two sectors (this detector error model has one)");
    const int n0 = P->sec[0].g->n, n1 = P->sec[1].g->n;
    QLDPC_REQUIRE(n_links >= 0, "n_links = %lld is negative", (long long)n_links);
    QLDPC_REQUIRE(link_ptr != nullptr || n_links == 0, "link_ptr is NULL but n_links = %lld", (long long)n_links);
    std::vector<int32_t> ptr((size_t)n1 + 1, 0);                          // no tables: every run is empty
    if (link_ptr) ptr.assign(link_ptr, link_ptr + n1 + 1);
    QLDPC_REQUIRE(ptr[n1] == n_links, "link_ptr[%d] = %d, not n_links = %lld", n1, ptr[n1], (long long)n_links);
    if ((rc = shotprior_check_links(n1, n0, ptr.data(), link_src, link_llr)) != QLDPC_OK) return rc;
    for (int j = 0; base_x && j < n1; j++) QLDPC_REQUIRE(std::isfinite(base_x[j]), "base_x[%d] is not finite", j);
    if ((rc = inputs_supported(P, shotprior_check_params(alpha, P->clip, P->max_iter),
                               [](const qldpc_graph *g) { return shotprior_mode(g) ? QLDPC_OK : shotprior_unsupported(g); })) != QLDPC_OK)
        return rc;
    QLDPC_USE_DEVICE(P->device);
    QLDPC_HIP_TRY(hipDeviceSynchronize());                              // a decode that is still enqueued reads the tables replaced here
    const std::vector<int32_t> src(link_src, link_src + n_links);
    const std::vector<double> llr(link_llr, link_llr + n_links), base(base_x, base_x + (base_x ? n1 : 0));
    DevBuf d_ptr, d_src, d_llr, d_base;                                  // all four or none: a failed upload leaves the plan's tables as they were
    if ((rc = upload(d_ptr, ptr)) || (rc = upload(d_src, src)) || (rc = upload(d_llr, llr)) || (rc = upload(d_base, base))) return rc;
    P->d_cl_ptr = std::move(d_ptr); P->d_cl_src = std::move(d_src); P->d_cl_llr = std::move(d_llr); P->d_cl_base = std::move(d_base);
    P->corr_alpha = alpha;
    P->corr_base = base_x != nullptr;
    P->path = Path::CORRELATED;
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_circuit_plan_use_f32(qldpc_circuit_plan *P) {
    int rc = switch_allowed(P, Path::F32);
    if (rc != QLDPC_OK || P->path == Path::F32) return rc;                  // asked again: nothing to replace
    rc = build_handles(P, &Sector::f32, [&](const Sector &S, int, qldpc_minsum32_decoder **out) {
        return minsum32_decoder_create_tab(S.g, S.h_prior.data(), P->max_iter, S.h_alpha, P->clip, P->flags & QLDPC_FLAG_PUBLIC_MASK, out);
    });
    if (rc == QLDPC_OK) P->path = Path::F32;
    return rc;
}

// The rules of the sampler axis, once.  qldpc_circuit_plan_use_fixed_weight, _use_erasure_noise, _use_noise_model and _use_soft_readout move a plan
// along it, and unlike the decode axes it is two-way: each of them also switches its sampler off again.
//   It asks no decode-path rule (switch_allowed is not consulted): what a trial is drawn with and what decodes it are independent.
//   Every sampler other than the independent draws refuses every other such sampler until it is switched off.  Asking again for the sampler the plan
//     is on brings new arguments.
//   Erasure noise, a noise model and soft readout need a circuit plan: a detector error model has no gate locations.
//   A fixed weight on a detector error model needs one probability for all mechanisms (dem_odd < 0).
// Launch arguments travel by value, so batches already enqueued keep the sampler they were enqueued with.
// QLDPC_OK, or QLDPC_ERR_INVALID with the error text set.
static int sampler_switch_allowed(const qldpc_circuit_plan *P, Sampler to) {
    static const char *const name[] = {"the independent draws", "a fixed weight", "erasure noise", "a noise model", "soft readout"};
    static const char *const the[] = {"", "the fixed weight", "erasure noise", "the noise model", "soft readout"};
    QLDPC_REQUIRE(!P->dem || to == Sampler::FIXED_WEIGHT, "%s needs a circuit plan: a detector error model has no gate locations", name[(int)to]);
    QLDPC_REQUIRE(P->sampler == Sampler::INDEPENDENT || P->sampler == to, "the plan samples %s: %s goes with the independent draws alone (switch %s off first)",
                  name[(int)P->sampler], name[(int)to], the[(int)P->sampler]);
    QLDPC_REQUIRE(to != Sampler::FIXED_WEIGHT || !P->dem || P->dem_odd < 0, "mechanism %lld of the detector error model does not have the probability of mechanism 0: fixed-weight "
                  "sampling needs one probability for all mechanisms (a non-uniform model has no weight strata)", (long long)P->dem_odd);
    return QLDPC_OK;
}
// Switching off a sampler the plan is not on changes nothing and is no error: only the plan's own sampler falls back to the independent draws, so
// "erasure noise off" leaves a plan on a noise model on its noise model.
static int sampler_off(qldpc_circuit_plan *P, Sampler which) {
    if (P->sampler == which) P->sampler = Sampler::INDEPENDENT;
    return QLDPC_OK;
}
// The order in which errors win inside an entry is part of its contract: a fixed weight checks its argument before the axis rules; the other three ask
// the axis rules (a circuit plan, then the refusals) before their arguments.  Every entry sets the plan's state after its last check, so a refused call
// leaves the plan sampling exactly what it sampled before.

// weight -1 = off
QLDPC_EXPORT int qldpc_circuit_plan_use_fixed_weight(qldpc_circuit_plan *P, int weight) {
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    if (weight == -1) return sampler_off(P, Sampler::FIXED_WEIGHT);
    int rc = fixed_weight_check(P->n_locs, weight);
    if (rc != QLDPC_OK || (rc = sampler_switch_allowed(P, Sampler::FIXED_WEIGHT)) != QLDPC_OK) return rc;
    P->fixed_weight = weight;
    P->sampler = Sampler::FIXED_WEIGHT;
    return QLDPC_OK;
}

// rate[op code], NULL = off
QLDPC_EXPORT int qldpc_circuit_plan_use_erasure_noise(qldpc_circuit_plan *P, const double rate[7]) {
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    if (rate == nullptr) return sampler_off(P, Sampler::ERASURE);
    int rc = sampler_switch_allowed(P, Sampler::ERASURE);
    if (rc != QLDPC_OK) return rc;
    uint32_t thr[8];
    if ((rc = erasure_rates_check(rate, thr)) != QLDPC_OK || (rc = erasure_sample_supported(P->sec[0].nsyn, P->sec[1].nsyn, P->n_locs)) != QLDPC_OK) return rc;
    QLDPC_USE_DEVICE(P->device);
    if ((rc = P->d_erased.ensure((size_t)P->batch * ((size_t)(P->n_locs + 31) / 32) * 4 + 4)) != QLDPC_OK) return rc;
    std::copy(thr, thr + 8, P->ethr);
    P->sampler = Sampler::ERASURE;
    return QLDPC_OK;
}

// NULL = off
QLDPC_EXPORT int qldpc_circuit_plan_use_noise_model(qldpc_circuit_plan *P, const qldpc_noise_model *model) {
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    if (model == nullptr) return sampler_off(P, Sampler::NOISE_MODEL);
    int rc = sampler_switch_allowed(P, Sampler::NOISE_MODEL);
    if (rc != QLDPC_OK) return rc;
    NoiseModelHost nm;
    if ((rc = noise_model_check(model, &nm)) != QLDPC_OK) return rc;
    if (!P->d_loc_cls.p) {                                               // the first switch: pack the classes the plan already holds on the device
        QLDPC_USE_DEVICE(P->device);
        std::vector<uint8_t> loc_type((size_t)P->n_locs);
        if (P->n_locs) QLDPC_HIP_TRY(hipMemcpy(loc_type.data(), P->d_loc_type.p, loc_type.size(), hipMemcpyDeviceToHost));
        DevBuf cls;
        if ((rc = upload(cls, noise_model_pack_classes(loc_type))) != QLDPC_OK) return rc;
        P->d_loc_cls = std::move(cls);
    }
    P->nm = nm;
    P->sampler = Sampler::NOISE_MODEL;
    return QLDPC_OK;
}

// What both soft switches need of a circuit plan, once: the packed classes (as the noise model's sampler reads them), the rank of every MeasX / MeasZ
// location among them and their number.  All or none.
static int soft_prepare(qldpc_circuit_plan *P) {
    if (P->n_meas >= 0) return QLDPC_OK;
    QLDPC_USE_DEVICE(P->device);
    std::vector<uint8_t> loc_type((size_t)P->n_locs);
    if (P->n_locs) QLDPC_HIP_TRY(hipMemcpy(loc_type.data(), P->d_loc_type.p, loc_type.size(), hipMemcpyDeviceToHost));
    std::vector<int32_t> rank(std::max<size_t>(loc_type.size(), 1), -1);
    int n_meas = 0;
    for (size_t l = 0; l < loc_type.size(); l++)
        if (loc_type[l] == C_OP_MEAS_X || loc_type[l] == C_OP_MEAS_Z) rank[l] = n_meas++;
    int rc;
    DevBuf cls, rk;
    if ((rc = upload(rk, rank)) != QLDPC_OK) return rc;
    if (!P->d_loc_cls.p) {
        if ((rc = upload(cls, noise_model_pack_classes(loc_type))) != QLDPC_OK) return rc;
        P->d_loc_cls = std::move(cls);
    }
    P->d_meas_rank = std::move(rk);
    P->n_meas = n_meas;
    return QLDPC_OK;
}
static size_t levels_bytes(const qldpc_circuit_plan *P) { return (size_t)P->batch * (size_t)P->n_meas + 4; }

// flip_mass NULL = off
QLDPC_EXPORT int qldpc_circuit_plan_use_soft_readout(qldpc_circuit_plan *P, int32_t levels, const double *flip_mass, const double *keep_mass) {
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    if (flip_mass == nullptr) return sampler_off(P, Sampler::SOFT);
    int rc = sampler_switch_allowed(P, Sampler::SOFT);
    if (rc != QLDPC_OK) return rc;
    SoftReadoutHost sr;
    if ((rc = soft_readout_check(levels, flip_mass, keep_mass, &sr)) != QLDPC_OK) return rc;
    QLDPC_REQUIRE(P->path != Path::SOFT || P->soft_levels == levels, "the plan decodes soft-aware with tables for %d levels: a readout with %d levels does not go with them",
                  P->soft_levels, levels);
    if ((rc = soft_prepare(P)) != QLDPC_OK) return rc;
    QLDPC_USE_DEVICE(P->device);
    if ((rc = P->d_levels.ensure(levels_bytes(P))) != QLDPC_OK) return rc;
    P->sr = sr;
    P->sampler = Sampler::SOFT;
    return QLDPC_OK;
}

// One sector's tables of qldpc_circuit_plan_use_soft_aware (host pointers).
struct SoftTabIn { const int32_t *meas_col, *meas_w, *lut_ptr; const double *lut; };

QLDPC_EXPORT int qldpc_circuit_plan_use_soft_aware(qldpc_circuit_plan *P, double alpha, int32_t levels, const int32_t *meas_col_z, const int32_t *meas_w_z,
                                                   const int32_t *lut_ptr_z, const double *lut_z, const int32_t *meas_col_x, const int32_t *meas_w_x,
                                                   const int32_t *lut_ptr_x, const double *lut_x) {
    int rc = switch_allowed(P, Path::SOFT);
    if (rc != QLDPC_OK) return rc;
    QLDPC_REQUIRE(!P->dem, "soft-aware decoding needs a circuit plan: a detector error model has no measurement locations to read levels from");
    QLDPC_REQUIRE(P->sampler != Sampler::SOFT || P->sr.levels == levels, "the plan samples soft readout with %d levels: tables for %d levels do not go with it", P->sr.levels, levels);
    if ((rc = soft_prepare(P)) != QLDPC_OK) return rc;
    const SoftTabIn in[2] = {{meas_col_z, meas_w_z, lut_ptr_z, lut_z}, {meas_col_x, meas_w_x, lut_ptr_x, lut_x}};
    for (int i = 0; i < 2; i++) {
        const Sector &S = P->sec[i];
        QLDPC_REQUIRE(in[i].lut_ptr && in[i].lut && (P->n_meas == 0 || (in[i].meas_col && in[i].meas_w)), "sector %c: meas_col, meas_w, lut_ptr or lut is NULL", "ZX"[i]);
        if ((rc = soft_check_tables(levels, P->n_meas, in[i].meas_col, in[i].meas_w, S.g->n, in[i].lut_ptr, in[i].lut)) != QLDPC_OK) {
            const std::string why = qldpc_last_error();
            set_error("sector %c: %s", "ZX"[i], why.c_str());
            return rc;
        }
        for (int j = 0; j < S.g->n; j++)      // a run of length 1 is the plan's own prior, verbatim: a plan without levels decodes a column without measurements as ever
            QLDPC_REQUIRE(in[i].lut_ptr[j + 1] - in[i].lut_ptr[j] != 1 || std::memcmp(&in[i].lut[in[i].lut_ptr[j]], &S.h_prior[j], 8) == 0,
                          "sector %c: lut[lut_ptr[%d]] = %.17g is not the plan's prior %.17g of column %d, which has no measurement", "ZX"[i], j,
                          in[i].lut[in[i].lut_ptr[j]], S.h_prior[j], j);
        if ((rc = soft_prior_supported(S.g->n)) != QLDPC_OK) return rc;
    }
    if ((rc = inputs_supported(P, shotprior_check_params(alpha, P->clip, P->max_iter),
                               [](const qldpc_graph *g) { return shotprior_mode(g) ? QLDPC_OK : shotprior_unsupported(g); })) != QLDPC_OK)
        return rc;
    QLDPC_USE_DEVICE(P->device);
    QLDPC_HIP_TRY(hipDeviceSynchronize());                              // a decode that is still enqueued reads the tables replaced here
    DevBuf nb[2][4];                                                     // all or none: a failed upload leaves the plan's tables as they were
    for (int i = 0; i < 2; i++) {
        const size_t nm = (size_t)P->n_meas, n = (size_t)P->sec[i].g->n;
        if ((rc = upload(nb[i][0], nm ? std::vector<int32_t>(in[i].meas_col, in[i].meas_col + nm) : std::vector<int32_t>(1, -1))) ||
            (rc = upload(nb[i][1], nm ? std::vector<int32_t>(in[i].meas_w, in[i].meas_w + nm) : std::vector<int32_t>(1, 1))) ||
            (rc = upload(nb[i][2], std::vector<int32_t>(in[i].lut_ptr, in[i].lut_ptr + n + 1))) ||
            (rc = upload(nb[i][3], std::vector<double>(in[i].lut, in[i].lut + in[i].lut_ptr[n]))))
            return rc;
    }
    for (int i = 0; i < 2; i++)
        if ((rc = P->sec[i].d_eprior.ensure((size_t)P->batch * (size_t)P->sec[i].g->n * 8)) != QLDPC_OK) return rc;
    if ((rc = P->d_levels.ensure(levels_bytes(P))) != QLDPC_OK) return rc;
    for (int i = 0; i < 2; i++) {
        Sector &S = P->sec[i];
        S.d_so_col = std::move(nb[i][0]); S.d_so_w = std::move(nb[i][1]); S.d_so_lutptr = std::move(nb[i][2]); S.d_so_lut = std::move(nb[i][3]);
    }
    P->soft_alpha = alpha;
    P->soft_levels = levels;
    P->path = Path::SOFT;
    return QLDPC_OK;
}

// qldpc_circuit_plan_sample plus the level record and, where asked for, the per-shot priors of both sectors (host pointers)
QLDPC_EXPORT int qldpc_circuit_plan_sample_soft(qldpc_circuit_plan *P, uint64_t seed, int64_t trial_begin, int64_t count, int8_t *sparse_z, int8_t *true_z,
                                                int8_t *sparse_x, int8_t *true_x, uint8_t *level, double *prior_z, double *prior_x) {
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    QLDPC_REQUIRE(!P->dem, "sample_soft needs a circuit plan: a detector error model has no measurement locations");
    QLDPC_REQUIRE(count >= 0 && trial_begin >= 0, "negative trial range");
    QLDPC_REQUIRE((prior_z == nullptr) == (prior_x == nullptr), "prior_z and prior_x are both NULL or both given");
    QLDPC_REQUIRE(!prior_z || P->path == Path::SOFT, "the per-shot priors need the tables of qldpc_circuit_plan_use_soft_aware");
    int rc = soft_prepare(P);
    if (rc != QLDPC_OK) return rc;
    QLDPC_REQUIRE(count == 0 || (sparse_z && true_z && sparse_x && true_x && (level || P->n_meas == 0)), "NULL output");
    QLDPC_USE_DEVICE(P->device);
    if ((rc = P->d_levels.ensure(levels_bytes(P))) != QLDPC_OK) return rc;
    int8_t *const sparse[2] = {sparse_z, sparse_x}, *const truth[2] = {true_z, true_x};
    double *const prior[2] = {prior_z, prior_x};
    return sample_readback(P, seed, trial_begin, count, sparse, truth, {P->d_levels.p, (size_t)P->n_meas, level, P->sampler != Sampler::SOFT},
                           prior_z ? launch_soft_prior : nullptr, prior);
}

// One sector's tables of qldpc_circuit_plan_use_erasure_aware (host pointers).
struct ErasureTabIn { const int32_t *loc_ptr, *loc_col; const uint8_t *loc_h; const int32_t *lut_ptr; const double *lut; };

QLDPC_EXPORT int qldpc_circuit_plan_use_erasure_aware(qldpc_circuit_plan *P, double alpha, const int32_t *loc_ptr_z, const int32_t *loc_col_z,
                                                      const uint8_t *loc_h_z, const int32_t *lut_ptr_z, const double *lut_z, const int32_t *loc_ptr_x,
                                                      const int32_t *loc_col_x, const uint8_t *loc_h_x, const int32_t *lut_ptr_x, const double *lut_x) {
    int rc = switch_allowed(P, Path::ERASURE);
    if (rc != QLDPC_OK) return rc;
    QLDPC_REQUIRE(!P->dem, "erasure-aware decoding needs a circuit plan: a detector error model has no gate locations to herald");
    const ErasureTabIn in[2] = {{loc_ptr_z, loc_col_z, loc_h_z, lut_ptr_z, lut_z}, {loc_ptr_x, loc_col_x, loc_h_x, lut_ptr_x, lut_x}};
    for (int i = 0; i < 2; i++) {
        const Sector &S = P->sec[i];
        QLDPC_REQUIRE(in[i].loc_ptr && in[i].lut_ptr && in[i].lut, "sector %c: loc_ptr, lut_ptr or lut is NULL", "ZX"[i]);
        if ((rc = erasure_check_tables(P->n_locs, in[i].loc_ptr, in[i].loc_col, in[i].loc_h, S.g->n, in[i].lut_ptr, in[i].lut)) != QLDPC_OK) return rc;
        for (int j = 0; j < S.g->n; j++)      // entry 0 of a column's run is the plan's own prior, verbatim: a shot without heralds decodes as the plan does
            QLDPC_REQUIRE(std::memcmp(&in[i].lut[in[i].lut_ptr[j]], &S.h_prior[j], 8) == 0, "sector %c: lut[lut_ptr[%d]] = %.17g is not the plan's prior %.17g of column %d",
                          "ZX"[i], j, in[i].lut[in[i].lut_ptr[j]], S.h_prior[j], j);
        if ((rc = erasure_prior_supported(S.g->n)) != QLDPC_OK) return rc;
    }
    if ((rc = inputs_supported(P, shotprior_check_params(alpha, P->clip, P->max_iter),
                               [](const qldpc_graph *g) { return shotprior_mode(g) ? QLDPC_OK : shotprior_unsupported(g); })) != QLDPC_OK)
        return rc;
    QLDPC_USE_DEVICE(P->device);
    QLDPC_HIP_TRY(hipDeviceSynchronize());                              // a decode that is still enqueued reads the tables replaced here
    DevBuf nb[2][5];                                                     // all or none: a failed upload leaves the plan's tables as they were
    for (int i = 0; i < 2; i++) {
        const size_t ne = (size_t)in[i].loc_ptr[P->n_locs], n = (size_t)P->sec[i].g->n;
        if ((rc = upload(nb[i][0], std::vector<int32_t>(in[i].loc_ptr, in[i].loc_ptr + P->n_locs + 1))) ||
            (rc = upload(nb[i][1], std::vector<int32_t>(in[i].loc_col, in[i].loc_col + ne))) ||
            (rc = upload(nb[i][2], std::vector<uint8_t>(in[i].loc_h, in[i].loc_h + ne))) ||
            (rc = upload(nb[i][3], std::vector<int32_t>(in[i].lut_ptr, in[i].lut_ptr + n + 1))) ||
            (rc = upload(nb[i][4], std::vector<double>(in[i].lut, in[i].lut + in[i].lut_ptr[n]))))
            return rc;
    }
    for (int i = 0; i < 2; i++)
        if ((rc = P->sec[i].d_eprior.ensure((size_t)P->batch * (size_t)P->sec[i].g->n * 8)) != QLDPC_OK) return rc;
    if ((rc = P->d_erased.ensure((size_t)P->batch * ((size_t)(P->n_locs + 31) / 32) * 4 + 4)) != QLDPC_OK) return rc;
    for (int i = 0; i < 2; i++) {
        Sector &S = P->sec[i];
        S.d_er_ptr = std::move(nb[i][0]); S.d_er_col = std::move(nb[i][1]); S.d_er_h = std::move(nb[i][2]);
        S.d_er_lutptr = std::move(nb[i][3]); S.d_er_lut = std::move(nb[i][4]);
    }
    P->era_alpha = alpha;
    P->path = Path::ERASURE;
    return QLDPC_OK;
}

// qldpc_circuit_plan_sample plus the herald record and, where asked for, the per-shot priors of both sectors (host pointers)
QLDPC_EXPORT int qldpc_circuit_plan_sample_erasures(qldpc_circuit_plan *P, uint64_t seed, int64_t trial_begin, int64_t count, int8_t *sparse_z,
                                                    int8_t *true_z, int8_t *sparse_x, int8_t *true_x, uint32_t *erased, double *prior_z, double *prior_x) {
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    QLDPC_REQUIRE(!P->dem, "sample_erasures needs a circuit plan: a detector error model has no gate locations to erase");
    QLDPC_REQUIRE(count >= 0 && trial_begin >= 0, "negative trial range");
    QLDPC_REQUIRE(count == 0 || (sparse_z && true_z && sparse_x && true_x && erased), "NULL output");
    QLDPC_REQUIRE((prior_z == nullptr) == (prior_x == nullptr), "prior_z and prior_x are both NULL or both given");
    QLDPC_REQUIRE(!prior_z || P->path == Path::ERASURE, "the per-shot priors need the tables of qldpc_circuit_plan_use_erasure_aware");
    QLDPC_USE_DEVICE(P->device);
    const size_t nw = (size_t)(P->n_locs + 31) / 32;
    if (const int rc = P->d_erased.ensure((size_t)P->batch * nw * 4 + 4); rc != QLDPC_OK) return rc;
    int8_t *const sparse[2] = {sparse_z, sparse_x}, *const truth[2] = {true_z, true_x};
    double *const prior[2] = {prior_z, prior_x};
    return sample_readback(P, seed, trial_begin, count, sparse, truth, {P->d_erased.p, nw * 4, erased, P->sampler != Sampler::ERASURE},
                           prior_z ? launch_erasure_prior : nullptr, prior);
}

// ---- recorded detection events in place of the sampler (kernels: events.hip) ----
static const int kMaxEventBits = 131070;           // two sectors of at most 65535 detectors

static int event_bits(const qldpc_circuit_plan *P) { return P->ev_bits ? P->ev_bits : P->sec[0].nsyn + (P->nsec == 2 ? P->sec[1].nsyn : 0); }
static EventsSector events_view(const qldpc_circuit_plan *P, int i) {
    const Sector &S = P->sec[i];
    if (i >= P->nsec) return EventsSector{0, 0, nullptr, nullptr};
    const int base = P->ev_bits ? S.ev_base : (i ? P->sec[0].nsyn : 0);
    return EventsSector{S.nsyn, base, S.ev_tab ? S.d_evtab.as<int32_t>() : (const int32_t *)nullptr, S.d_syn.as<int8_t>()};
}

QLDPC_EXPORT int qldpc_circuit_plan_set_event_layout(qldpc_circuit_plan *P, int32_t n_bits, const int32_t *bit_of_row0, const int32_t *bit_of_row1) {
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    QLDPC_REQUIRE(n_bits >= 1 && n_bits <= kMaxEventBits, "n_bits = %d is outside 1..%d", n_bits, kMaxEventBits);
    const int32_t *const tab[2] = {bit_of_row0, bit_of_row1};
    bool is_tab[2] = {false, false};
    int base[2] = {0, P->sec[0].nsyn};
    for (int i = 0; i < P->nsec; i++) {
        const int nsyn = P->sec[i].nsyn;
        if (!tab[i]) {
            QLDPC_REQUIRE(base[i] + nsyn <= n_bits, "n_bits = %d is too small for the default layout of sector %d (bits %d..%d)", n_bits, i, base[i], base[i] + nsyn - 1);
            continue;
        }
        bool run = tab[i][0] >= 0;
        for (int r = 0; r < nsyn; r++) {
            QLDPC_REQUIRE(tab[i][r] >= -1 && tab[i][r] < n_bits, "bit_of_row%d[%d] = %d is outside -1..%d (n_bits = %d)", i, r, tab[i][r], n_bits - 1, n_bits);
            run = run && tab[i][r] == tab[i][0] + r;
        }
        is_tab[i] = !run;                                              // a contiguous run of bits needs no table
        if (run) base[i] = tab[i][0];
    }
    QLDPC_USE_DEVICE(P->device);
    int rc = QLDPC_OK;
    QLDPC_HIP_TRY(hipDeviceSynchronize());                              // a decode that is still enqueued reads the tables replaced here
    for (int i = 0; i < P->nsec; i++)
        if (is_tab[i] && (rc = upload(P->sec[i].d_evtab, std::vector<int32_t>(tab[i], tab[i] + P->sec[i].nsyn))) != QLDPC_OK) return rc;
    for (int i = 0; i < P->nsec; i++) { P->sec[i].ev_tab = is_tab[i]; P->sec[i].ev_base = base[i]; }
    P->ev_bits = n_bits;
    return QLDPC_OK;
}

// what decode_events and unpack_events check alike
static int events_args(const qldpc_circuit_plan *P, const uint8_t *events, int64_t stride) {
    QLDPC_REQUIRE(events != nullptr, "events is NULL");
    const int nbytes = (event_bits(P) + 7) / 8;
    QLDPC_REQUIRE(stride >= nbytes, "stride = %lld is below the %d bytes of a record (n_bits = %d)", (long long)stride, nbytes, event_bits(P));
    QLDPC_REQUIRE(stride <= ((int64_t)1 << 30), "stride = %lld is above 2^30 bytes", (long long)stride);
    return QLDPC_OK;
}

// one pass over the records [0, count): copy (host records) + unpack in the sampler's bracket, the sectors' decode as in a run, predict in the judge's bracket.
// host = true: events / pred0 / pred1 / flags are host pointers, and every batch is copied back and waited for (as circuit_run does for its outcomes);
// host = false: device pointers, everything is enqueued on s and nothing is waited for.
// scored: `score` (uint64[count], host or device like the rest) receives the confidence of every shot; there is no outcome, so the histogram stays as it is.
static int decode_events(qldpc_circuit_plan *P, uint64_t seed, int64_t shot_begin, int64_t count, const uint8_t *events, int64_t stride, hipStream_t s,
                         uint64_t *pred0, uint64_t *pred1, uint8_t *flags, bool host, bool scored = false, uint64_t *score = nullptr) {
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    QLDPC_REQUIRE(!scored || P->conf_kind >= 0, "the plan has no confidence (qldpc_circuit_plan_use_confidence)");
    QLDPC_REQUIRE(!scored || count == 0 || score != nullptr, "score is NULL");
    QLDPC_REQUIRE(count >= 0, "count is negative");
    QLDPC_REQUIRE(shot_begin >= 0, "shot_begin is negative");
    if (count == 0) return QLDPC_OK;
    int rc = events_args(P, events, stride);
    if (rc != QLDPC_OK) return rc;
    const bool two = P->nsec == 2;
    QLDPC_REQUIRE(pred0 != nullptr, "pred0 is NULL");
    QLDPC_REQUIRE(pred1 != nullptr || !two, "pred1 is NULL (the plan has two sectors)");
    QLDPC_REQUIRE(flags != nullptr, "flags is NULL");
    QLDPC_USE_DEVICE(P->device);
    const size_t Bz = (size_t)P->batch;
    if (host) {
        if ((rc = P->d_events.ensure(Bz * (size_t)stride)) || (rc = P->d_evflags.ensure(Bz)) || (rc = ensure_each(P, &Sector::d_pred, Bz * 8))) return rc;
        if (!two && pred1) std::memset(pred1, 0, (size_t)count * 8);
    } else if (!two && pred1) {
        QLDPC_HIP_TRY(hipMemsetAsync(pred1, 0, (size_t)count * 8, s));
    }
    const JudgeSector Z = judge_view(P->sec[0]), X = two ? judge_view(P->sec[1]) : JudgeSector{};
    const EventsSector E0 = events_view(P, 0), E1 = events_view(P, 1);
    const int n_bits = event_bits(P);
    for (int64_t off = 0; off < count; off += P->batch) {
        const int64_t B = std::min<int64_t>(P->batch, count - off);
        if (P->pending.size() > 256) drain_phases(P, false);
        if ((rc = phase_mark(P, QLDPC_PHASE_SAMPLE, s, true)) != QLDPC_OK) return rc;
        const uint8_t *d_rec = events + off * stride;
        if (host) {
            QLDPC_HIP_TRY(hipMemcpyAsync(P->d_events.p, d_rec, (size_t)B * (size_t)stride, hipMemcpyHostToDevice, s));
            d_rec = P->d_events.as<uint8_t>();
        }
        if ((rc = events_unpack_launch(B, d_rec, stride, n_bits, E0, E1, two, P->d_count.as<int32_t>(), s)) != QLDPC_OK) return rc;
        if ((rc = phase_mark(P, QLDPC_PHASE_SAMPLE, s, false)) != QLDPC_OK) return rc;
        for (int sector = 0; sector < P->nsec; sector++)
            if ((rc = decode_sector(P, sector, B, s, seed, shot_begin + off)) != QLDPC_OK) return rc;
        if ((rc = phase_mark(P, QLDPC_PHASE_JUDGE, s, true)) != QLDPC_OK) return rc;
        unsigned long long *p0 = host ? P->sec[0].d_pred.as<unsigned long long>() : reinterpret_cast<unsigned long long *>(pred0) + off;
        unsigned long long *p1 = !two ? nullptr : host ? P->sec[1].d_pred.as<unsigned long long>() : reinterpret_cast<unsigned long long *>(pred1) + off;
        uint8_t *fl = host ? P->d_evflags.as<uint8_t>() : flags + off;
        if ((rc = events_predict_launch(B, Z, X, two, p0, p1, fl, s)) != QLDPC_OK) return rc;
        if (scored) {
            if ((rc = launch_confidence(P, B, nullptr, s)) != QLDPC_OK) return rc;
            QLDPC_HIP_TRY(hipMemcpyAsync(score + off, P->d_score.p, (size_t)B * 8, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
        }
        if ((rc = phase_mark(P, QLDPC_PHASE_JUDGE, s, false)) != QLDPC_OK) return rc;
        P->batches++;
        if (host) {
            QLDPC_HIP_TRY(hipMemcpyAsync(pred0 + off, p0, (size_t)B * 8, hipMemcpyDeviceToHost, s));
            if (two) QLDPC_HIP_TRY(hipMemcpyAsync(pred1 + off, p1, (size_t)B * 8, hipMemcpyDeviceToHost, s));
            QLDPC_HIP_TRY(hipMemcpyAsync(flags + off, fl, (size_t)B, hipMemcpyDeviceToHost, s));
            QLDPC_HIP_TRY(hipStreamSynchronize(s));
        }
    }
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_circuit_plan_decode_events(qldpc_circuit_plan *P, uint64_t seed, int64_t shot_begin, int64_t count, const uint8_t *events,
                                                  int64_t stride, void *stream, uint64_t *pred0, uint64_t *pred1, uint8_t *flags) {
    return decode_events(P, seed, shot_begin, count, events, stride, reinterpret_cast<hipStream_t>(stream), pred0, pred1, flags, true);
}

QLDPC_EXPORT int qldpc_circuit_plan_decode_events_dev(qldpc_circuit_plan *P, uint64_t seed, int64_t shot_begin, int64_t count, const uint8_t *d_events,
                                                      int64_t stride, void *stream, uint64_t *d_pred0, uint64_t *d_pred1, uint8_t *d_flags) {
    return decode_events(P, seed, shot_begin, count, d_events, stride, reinterpret_cast<hipStream_t>(stream), d_pred0, d_pred1, d_flags, false);
}

QLDPC_EXPORT int qldpc_circuit_plan_decode_events_scored(qldpc_circuit_plan *P, uint64_t seed, int64_t shot_begin, int64_t count, const uint8_t *events,
                                                         int64_t stride, void *stream, uint64_t *pred0, uint64_t *pred1, uint8_t *flags, uint64_t *score) {
    return decode_events(P, seed, shot_begin, count, events, stride, reinterpret_cast<hipStream_t>(stream), pred0, pred1, flags, true, true, score);
}

QLDPC_EXPORT int qldpc_circuit_plan_decode_events_scored_dev(qldpc_circuit_plan *P, uint64_t seed, int64_t shot_begin, int64_t count, const uint8_t *d_events,
                                                             int64_t stride, void *stream, uint64_t *d_pred0, uint64_t *d_pred1, uint8_t *d_flags,
                                                             uint64_t *d_score) {
    return decode_events(P, seed, shot_begin, count, d_events, stride, reinterpret_cast<hipStream_t>(stream), d_pred0, d_pred1, d_flags, false, true, d_score);
}

// the unpacker alone, the counterpart of qldpc_circuit_plan_sample: sparse0 int8[count][nsyn0], sparse1 int8[count][nsyn1] (host; sparse1 may be NULL on one sector)
QLDPC_EXPORT int qldpc_circuit_plan_unpack_events(qldpc_circuit_plan *P, int64_t count, const uint8_t *events, int64_t stride, int8_t *sparse0, int8_t *sparse1) {
    QLDPC_REQUIRE(P != nullptr, "plan is NULL");
    QLDPC_REQUIRE(count >= 0, "count is negative");
    if (count == 0) return QLDPC_OK;
    int rc = events_args(P, events, stride);
    if (rc != QLDPC_OK) return rc;
    QLDPC_REQUIRE(sparse0 != nullptr, "sparse0 is NULL");
    QLDPC_REQUIRE(sparse1 != nullptr || P->nsec == 1, "sparse1 is NULL (the plan has two sectors)");
    QLDPC_USE_DEVICE(P->device);
    if ((rc = P->d_events.ensure((size_t)P->batch * (size_t)stride)) != QLDPC_OK) return rc;
    int8_t *const sparse[2] = {sparse0, sparse1};
    const EventsSector E0 = events_view(P, 0), E1 = events_view(P, 1);
    for (int64_t off = 0; off < count; off += P->batch) {
        const int64_t B = std::min<int64_t>(P->batch, count - off);
        QLDPC_HIP_TRY(hipMemcpy(P->d_events.p, events + off * stride, (size_t)B * (size_t)stride, hipMemcpyHostToDevice));
        if ((rc = events_unpack_launch(B, P->d_events.as<uint8_t>(), stride, event_bits(P), E0, E1, P->nsec == 2, nullptr, nullptr)) != QLDPC_OK) return rc;
        QLDPC_HIP_TRY(hipDeviceSynchronize());
        for (int i = 0; i < P->nsec; i++)
            QLDPC_HIP_TRY(hipMemcpy(sparse[i] + off * P->sec[i].nsyn, P->sec[i].d_syn.p, (size_t)B * P->sec[i].nsyn, hipMemcpyDeviceToHost));
    }
    return QLDPC_OK;
}

QLDPC_EXPORT void qldpc_circuit_plan_destroy(qldpc_circuit_plan *P) { delete P; }
