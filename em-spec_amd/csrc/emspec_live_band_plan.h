// emspec_live_band_plan.h — internal: the host arithmetic of a live MULTI-BAND session (emspec_columns_multiband /
// emspec_push_samples_multiband): the K bands of emspec_band_plan.h on the streaming session of
// emspec_live_plan.h.  The session's counters, descriptors and push / flush / frame steps are the single-resolution ones at
// n = n[0] (`g` below); this header adds what each band's frame launch and column ring need, and the rule that decides between
// finalising in place and the one finalize kernel for all bands.  Integer arithmetic only.  No HIP, nothing of the engine:
// tests/test_live_band_plan_cpu.py runs it through a stand-alone program (tests/cdriver/live_band_plan_driver.cpp).
#pragma once
#include "emspec_band_plan.h"
#include "emspec_live_plan.h"

namespace emspec {

// One band of the session: rows [lo, hi) of the output column from fft size n.  Its frames run frame_shift ahead of the long
// band's, its frame j sits on emitted column j - shift, and its ring is indexed by the emitted column.
struct LiveBand {
    int n = 0, lo = 0, hi = 0;
    int shift = 0;         // (n[0] - n) / (2 hop)
    int D = 0;             // latency(n, hop, reassign): the band's own
    int frame_shift = 0;   // 2 shift
    int lat_extra = 0;     // D_0 - D: what the frame kernel adds to its plan's D to finalise the emitted column
    int slots = 0;         // column-ring slots per stream: mmax + shift + D_0 + D (band 0: 2 D_0 + mmax)
    int rows() const { return hi - lo; }
};

struct LiveBandGeometry {
    LiveGeometry g;        // the session at n[0], single-resolution form: mmax, cap, ring_mask, D, the staging and output sizes
    int bands = 0;         // 0: not a multi-band session
    LiveBand b[kMaxBands];
    // Every size below is in bytes.  Band k's column ring, per stream and of all S streams: [slots][rows] cells
    size_t ring_bytes(int k, size_t cell) const { return (size_t)b[k].slots * b[k].rows() * cell; }
    size_t rings_bytes(int k, size_t cell) const { return (size_t)g.S * ring_bytes(k, cell); }
    size_t done_bytes() const { return (size_t)g.S * 4 * bands; }   // arrival counters, one set per band: band k's at done + k S
    // the workgroups per stream of band k's frame launch, without the ingest workgroup: on a stream's first frame (priming) the
    // band transforms frames 0 .. 2 shift at once
    int launch_frames(int k, int frames, bool priming) const { return frames + (priming ? b[k].frame_shift : 0); }
    // The finalize rule.  A band alone would defer its finalize to a second kernel when the launch completes more than
    // inline_max columns per stream or its transform is small (n < 2048: too few threads for 1024 rows).  When ANY band would,
    // EVERY band's frame launch only scatters and one kernel finalises all bands' rows: K + 1 launches, not up to 2 K.
    bool defers(int frames, int inline_max) const {
        if (frames > inline_max) return true;
        for (int k = 0; k < bands; ++k)
            if (b[k].n < 2048) return true;
        return false;
    }
    // the session was opened with these bands (sizes and split rows; hop, reassign, S and the form are g's)
    bool same_bands(const BandPlan& p) const {
        if (p.bands != bands) return false;
        for (int k = 0; k < bands; ++k)
            if (p.n[k] != b[k].n || p.lo[k] != b[k].lo || p.hi[k] != b[k].hi) return false;
        return true;
    }
};

// p: an accepted band plan (band_shape_error and band_split_error both null)
inline LiveBandGeometry live_band_geometry(int S, const BandPlan& p, int hop, int reassign, int form) {
    LiveBandGeometry m;
    m.g = live_geometry(S, p.n[0], hop, reassign, form);
    m.bands = p.bands;
    // Band k's frames run 2 shift ahead and its ring is indexed by the emitted column.  A call that feeds long frames
    // j .. j + m - 1 finds emitted columns >= j - D unfinalised, and the band's last frame, j + m - 1 + 2 shift = emitted column
    // j + m - 1 + shift, adds up to D_k columns further: m + shift + D + D_k columns are live at once.
    for (int k = 0; k < p.bands; ++k) {
        LiveBand& b = m.b[k];
        b.n = p.n[k]; b.lo = p.lo[k]; b.hi = p.hi[k];
        b.shift = p.shift[k];
        b.D = latency(p.n[k], hop, reassign);
        b.frame_shift = 2 * b.shift;
        b.lat_extra = m.g.D - b.D;
        b.slots = m.g.mmax + b.shift + m.g.D + b.D;
    }
    return m;
}

}  // namespace emspec
