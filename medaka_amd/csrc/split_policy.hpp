// The split scan's call-level policy (scan_split.hpp, DESIGN.md sections 4.9 and 4.9b): options, margin learner, back-off,
// the fp32-parity probe of half precision, the audit cadence and verdict, and the record of the last call (mdk_gru_get_split).
// Host state only -- no device code, no device pointers.  Both GRU forward entries feed it: the synchronous one (run_forward)
// retires each call's verdict at once, the stream-ordered one (retire_one) when the call's record comes home.  The CPU tests
// drive it device-free through mdk_margin_sim.  Part of api.hip (included there before gru_model.hpp).
#pragma once
// ---- the margin, learned per model.  The margins a model can learn: a ladder instead of doublings (a set that needs 192 should
// not pay for 256: 19 % of all columns against 25 %).  Margins outside the ladder (option "scan_split_margin") join it at the next rung.
static const int kMarginLadder[] = {64, 96, 128, 192, 256, 384, 512};
static int split_margin_up(int G) {
    for (int r : kMarginLadder) if (r > G) return r;
    return 2 * kSplitMarginMax;                      // above the ladder: the caller gives the model up
}
static int split_margin_down(int G, int floor_) {
    int best = 0;
    for (int r : kMarginLadder) if (r < G && r >= floor_) best = r;
    return best;                                     // 0: nothing smaller is allowed
}
struct MarginLearner {
    int cur = 0;          // margin in use (0: the option's starting margin)
    int floor_ = 0;       // no shrink below this: one rung above the largest margin a certificate was ever rejected at
    int quiet = 0;        // consecutive certified calls at the current margin whose differences sat at the noise floor
    int trial_back = 0;   // != 0: the current margin is a shrink on trial; a rejection returns to this one
    enum Next { RETRY = 0, GIVE_UP = 1 };
    void reset(bool forget_rejections) { cur = quiet = trial_back = 0; if (forget_rejections) floor_ = 0; }
    // a certified call at margin G; returns the margin a kept trial came from (0: none).  `adapt` = quiet calls before a smaller
    // margin is tried (0: never), `noise_floor` = largest junction difference that still counts as quiet
    int certified(int G, float worst, float noise_floor, int adapt) {
        const int was = trial_back;
        trial_back = 0;
        quiet = worst <= noise_floor ? quiet + 1 : 0;
        if (adapt > 0 && quiet >= adapt) {
            const int down = split_margin_down(G, floor_);
            quiet = 0;
            if (down) { trial_back = G; cur = down; }
        }
        return was;
    }
    // a rejected certificate at margin G: RETRY = run the call again at `cur` (a failed trial goes back, anything else one rung
    // up), GIVE_UP = nothing larger is left.  `*back` = 1 if this was a trial
    Next rejected(int G, int *back) {
        quiet = 0;
        floor_ = std::max(floor_, split_margin_up(G));          // never shrink to a rejected margin again
        *back = 0;
        if (trial_back) { cur = trial_back; trial_back = 0; *back = 1; return RETRY; }
        const int next = split_margin_up(G);
        if (next > kSplitMarginMax) return GIVE_UP;
        cur = next;
        return RETRY;
    }
};

// ---- the policy.  A verdict of a call planned under a learner state that has moved since (a stream-ordered call enqueued before an
// earlier one's verdict was retired: another margin, a trial, the back-off) is not `current`: it is recorded and counted, but moves
// neither the learner nor the back-off.  Every retirement that moves them starts a new `learner_epoch`, and a stream-ordered call
// carries the epoch, precision and margin it was enqueued with.  So one episode of rejections moves the learner one step and starts
// ONE back-off however many calls were in flight (at the largest margin GIVE_UP leaves the margin where it was: without the epoch
// every call in flight would double the back-off again).  A synchronous call's verdict is retired at once: always current.
struct SplitPolicy {
    int opt_scan_split = 1;                  // 0 off, 1 auto, n >= 2: n chunks per window whenever the shape allows it
    int opt_split_margin = 128;              // G: columns of warm-up on either side of a chunk (where the model starts)
    MarginLearner margin;                    // the margin in use, LEARNED per model: one rung up the ladder 64 .. 512 on a rejected
                                             // certificate, one rung down after `opt_split_adapt` certified calls at the noise floor
    int opt_split_adapt = 8;                 // certified calls at the noise floor before a smaller margin is tried (0: never shrink)
    // half precision: a margin is used only after a call CERTIFIED AT IT IN FP32-PARITY MODE (a "probe": the same call, run once
    // more with the hi/lo operands, threshold 2^-18, result discarded) -- half mode's own certificate compares fp16 images of h
    // (threshold 2^-10) and cannot see an un-merged state below ~1e-3; see run_forward
    int opt_split_probe = 1;                 // 0: half mode trusts its own certificate (round 5's behaviour)
    std::vector<int> probed_ok;              // margins a probe certified
    long probes_done = 0;
    float probe_last_delta = 0.f;
    int probe_inflight_G = 0;                // stream-ordered: margin of the probe whose verdict sits on the device, not yet retired (0: none)
    bool split_disabled = false;             // a certificate failed at the largest margin (or an audit failed): sequential scans (auto mode)
    long split_retry_in = 0;                 // ... for this many calls; then one more try at the largest margin (0: for good -- failed audits)
    long split_backoff = 0;                  // the last back-off (doubles per rejection at the largest margin: 64 .. 4096 calls)
    long learner_epoch = 0;                  // bumped by every verdict that moves the margin learner or the back-off
    int opt_split_audit = 1;                 // 0 never, 1 the first certified call of every margin, 2 every certified call
    int split_audited_key = 0;               // margin | precision << 16 whose first certified call has been audited (0 = none yet)
    int audit_inflight_key = 0;              // stream-ordered: audit key of an audit enqueued and not yet retired
    // standing audit: every `opt_split_audit_every`-th certified call is ALSO run as the sequential scan
    int opt_split_audit_every = 256;
    long split_calls_since_audit = 0;
    long audits_done = 0;
    int audit_failures = 0;
    float audit_worst = 0.f;
    mdk_gru_split last_split{};              // the record of the last call (mdk_gru_get_split)

    // process-wide defaults (the options of the same names override them per model)
    void read_env() {
        if (const char *e = getenv("MDK_SCAN_SPLIT")) opt_scan_split = std::min(std::max(atoi(e), 0), kMaxSplit);
        if (const char *e = getenv("MDK_SCAN_SPLIT_ADAPT")) opt_split_adapt = std::max(atoi(e), 0);
        if (const char *e = getenv("MDK_SCAN_SPLIT_PROBE")) opt_split_probe = atoi(e) ? 1 : 0;
        if (const char *e = getenv("MDK_SCAN_SPLIT_MARGIN")) {
            const int g = atoi(e);
            if (g >= 16 && g <= 4096 && g % 8 == 0) opt_split_margin = g;
        }
    }
    // options "scan_split" (forget_rejections) and "scan_split_margin": a model that fell back is re-armed
    void rearm(bool forget_rejections) {
        margin.reset(forget_rejections);     // ("scan_split_margin": what the certificates rejected so far stays learned)
        if (forget_rejections) probed_ok.clear();
        split_disabled = false;
        split_retry_in = split_backoff = 0;
    }
    int margin_in_use() const { return margin.cur ? margin.cur : opt_split_margin; }
    bool is_current(long epoch, int precision, int G, int model_precision) const {
        return epoch == learner_epoch && precision == model_precision && margin_in_use() == G;
    }
    // A rejection at the largest margin may be the INPUT's doing (a zero-coverage run, a stretch the model was never trained on:
    // dynamics that do not forget THERE), not the model's: the split is tried again after a back-off of 64, 128, ... 4096 calls
    // (calls enqueued, on the stream-ordered entry), at the largest margin (one rejected forward per retry, < 1 % of the calls in
    // between).  The start of a call counts the back-off down; returns the call's status while it has not split.
    int begin_call() {
        if (split_disabled && split_retry_in > 0 && --split_retry_in == 0) { split_disabled = false; learner_epoch++; }
        return split_disabled ? MDK_SPLIT_DISABLED : MDK_SPLIT_NOT_USED;
    }
    bool backoff_ends_next_call() const { return split_disabled && split_retry_in == 1; }
    // the record of a call of T columns, not split (yet): the fallbacks carry over
    void open_record(int T, int status) {
        const int fallbacks = last_split.fallbacks;
        memset(&last_split, 0, sizeof(last_split));
        last_split.chunks = 1; last_split.columns = T; last_split.fallbacks = fallbacks;
        last_split.status = status;
        report();
    }
    // the certificate of a split call: S chunks of Tv columns at margin G, largest junction difference `worst`
    void record(int S, int G, int Tv, float worst, bool certified) {
        last_split.chunks = S; last_split.margin = G; last_split.columns = Tv;
        last_split.max_delta = worst;
        last_split.status = certified ? MDK_SPLIT_CERTIFIED : MDK_SPLIT_REJECTED;
    }
    // the next certified call is a periodic audit
    bool periodic_audit_next() const {
        return opt_split_audit == 1 && opt_split_audit_every > 0 && split_calls_since_audit + 1 >= opt_split_audit_every;
    }
    bool probe_due(int G, int precision) const {
        return precision == MDK_PREC_FP16 && opt_scan_split == 1 && opt_split_probe &&
               (std::find(probed_ok.begin(), probed_ok.end(), G) == probed_ok.end() || periodic_audit_next());
    }
    // a probe at margin G: `delta` = its largest junction difference.  A rejected probe is the call's certificate.
    void probed(int G, bool ok, float delta) {
        probes_done++;
        probe_last_delta = delta;
        probed_ok.erase(std::remove(probed_ok.begin(), probed_ok.end(), G), probed_ok.end());
        if (ok) probed_ok.push_back(G);
        if (probe_inflight_G == G) probe_inflight_G = 0;
        if (!ok) last_split.max_delta = delta;
        report();
    }
    void certified(int G, int precision, bool current) {
        if (!current) return;
        split_backoff = 0;
        // The margin is the split's price (12.8 % of all columns at 128, 5.7 % at 64) and what it has to be is the MODEL's
        // forgetting length: after `scan_split_adapt` certified calls in a row whose largest junction difference sat at the
        // rounding-noise floor (a quarter of the threshold), the next call tries one rung less.  A trial that is rejected
        // costs that one forward: the call is repeated at the margin that worked, and no shrink goes below it again.
        const int cur0 = margin.cur, trial0 = margin.trial_back;
        const float quiet_thr = 0.25f * (precision == MDK_PREC_FP16 ? kSplitEpsHalf : kSplitEps);
        const int was = margin.certified(G, last_split.max_delta, quiet_thr, opt_scan_split == 1 ? opt_split_adapt : 0);
        if (was) fprintf(stderr, "[medaka_amd] split scan: certified at a margin of %d columns (was %d): kept\n", G, was);
        if (margin.cur != cur0 || margin.trial_back != trial0) learner_epoch++;
    }
    // Audit.  The certificate argues from the states at the junctions; the audit looks at what is delivered: the call is ALSO run
    // as the sequential scan on the device and the two (B, T, C) results are compared in full.  Audited are the first certified
    // call of a model (and the first at every margin / precision it moves to) and, as a STANDING check on whatever input the model
    // meets later, every `scan_split_audit_every`-th certified call after that (default 256: one sequential forward of ~2x a split
    // forward's time per 256 calls, < 1 %; a concurrent low-priority audit was tried first and cost far more -- any second tenant
    // keeps the recurrence's work-groups from being resident together).  A mismatch delivers the sequential result and turns the
    // split off for the model.  Returns the audit's key (0: no audit); the stream-ordered entry asks at enqueue, for every split call.
    static int audit_key(int G, int precision) { return G | (precision << 16) | (1 << 24); }
    int audit_due(int G, int precision) {
        const int key = audit_key(G, precision);
        const bool first = split_audited_key != key && audit_inflight_key != key;
        const bool periodic = !first && opt_split_audit_every > 0 && ++split_calls_since_audit >= opt_split_audit_every;
        if (opt_split_audit == 0 || (opt_split_audit == 1 && !first && !periodic)) return 0;
        split_calls_since_audit = 0;
        return key;
    }
    // the audit of a certified call: `dp` = largest |p_split - p_sequential|; false: the sequential result is to be delivered
    bool audit_passed(int G, int precision, float dp) {
        audits_done++;
        audit_worst = std::max(audit_worst, dp);
        last_split.audited = 1;
        last_split.audit_max_dp = dp;
        const bool ok = dp <= (precision == MDK_PREC_FP16 ? kAuditTolHalf : kAuditTol);
        if (ok) {
            split_audited_key = audit_key(G, precision);
        } else {
            // never seen: certified junctions, different probabilities
            fprintf(stderr, "[medaka_amd] split scan: an audit found |p_split - p_sequential| = %.3g behind a certified split (margin %d): "
                            "the sequential result is delivered and the split scan is off for this model\n", dp, G);
            audit_failures++;
            last_split.status = MDK_SPLIT_REJECTED;
            last_split.fallbacks++;
            split_disabled = true;
            learner_epoch++;
        }
        report();
        return ok;
    }
    // A rejected certificate at margin G: some junction did not merge, this model remembers further back than the margin.  Auto
    // mode tries again with the next rung and keeps it for later calls (said once on stderr); the model is given up (sequential
    // scans, for a back-off) only by a rejection AT kSplitMarginMax: a very long or chaotic memory.  A forced chunk count is not
    // second-guessed.  Returns true if the call is to be repeated at margin_in_use() (synchronous entry; a shape that no longer
    // splits at the new margin is answered sequentially -- this call only).
    bool rejected(int G, bool current) {
        last_split.status = MDK_SPLIT_REJECTED;
        last_split.fallbacks++;
        if (!current) return false;
        margin.quiet = 0;
        if (opt_scan_split != 1) return false;
        int was_trial = 0;
        const MarginLearner::Next nx = margin.rejected(G, &was_trial);
        learner_epoch++;
        if (was_trial) {
            // a shrink on trial did not certify: back to the margin that did
            fprintf(stderr, "[medaka_amd] split scan: a margin of %d columns does not certify (junction states differ by %.3g): back to %d\n",
                    G, last_split.max_delta, margin.cur);
            return true;
        }
        if (nx == MarginLearner::GIVE_UP) {
            split_disabled = true;
            split_backoff = split_backoff ? std::min<long>(2 * split_backoff, 4096) : 64;
            split_retry_in = split_backoff;
            if (split_backoff == 64)
                fprintf(stderr, "[medaka_amd] split scan: junction states still differ by %.3g at a margin of %d columns: sequential scans "
                                "for the next %ld calls, then another try (back-off doubling up to 4096 calls)\n",
                        last_split.max_delta, G, split_backoff);
            return false;
        }
        fprintf(stderr, "[medaka_amd] split scan: junction states differed by %.3g at a margin of %d columns: margin %d from now on\n",
                last_split.max_delta, G, margin.cur);
        return true;
    }
    // may the verdict of the call in progress still move the next call's plan (a smaller margin on trial, an audit or probe due)?
    bool next_plan_may_move() const {
        if (opt_scan_split == 1 && opt_split_adapt > 0 && margin.quiet + 2 >= opt_split_adapt &&
            split_margin_down(margin_in_use(), margin.floor_) != 0) return true;
        if (margin.trial_back) return true;
        if (opt_scan_split && opt_split_audit == 1 &&
            (split_audited_key == 0 || (opt_split_audit_every > 0 && split_calls_since_audit + 2 >= opt_split_audit_every))) return true;
        return opt_split_audit == 2;
    }
    // the counters into the record (every method that moves one, and open_record, ends with this)
    void report() {
        last_split.audits = (int)std::min<long>(audits_done, 0x7fffffff);
        last_split.audit_failures = audit_failures;
        last_split.audit_worst_dp = audit_worst;
        last_split.probes = (int)std::min<long>(probes_done, 0x7fffffff);
        last_split.probe_max_delta = probe_last_delta;
    }
};
