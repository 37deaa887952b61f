// Server-side GPU-busy sampler for gpu-schd (lease accounting,
// MI355X-native).
//
// Charges each lease the GPU time it actually used instead of wall
// time: gpu-schd reads the device's GFX activity through librocm_smi64
// every few ms and credits the busy ms since the previous read to the
// current token holder (TokenScheduler::add_busy). Advantages over
// client-side hipEvent accounting (the alternative considered in
// round 1):
//   - zero per-dispatch overhead in the hook's hot path (an event
//     record per gated launch would cost ~2 us x thousands of
//     launches/step);
//   - a CPU-bound phase inside a lease (dataloader stall, sparse
//     dispatch) is NOT charged — quota error stays low for bursty
//     pods, not just saturating ones;
//   - measured on the host, outside the container: a hostile hook
//     cannot under-report.
//
// librocm_smi64 is dlopen'd so gpu-schd still builds and runs on
// CPU-only boxes (tests); without the library the scheduler keeps the
// round-1 wall/RET accounting.
#pragma once

#include <dlfcn.h>
#include <stdint.h>
#include <unistd.h>

#include <algorithm>

#include "../common/protocol.hpp"

namespace ks {

// Busy milliseconds from successive reads of gpu_busy_percent.
//
// The SMU does not report the instantaneous activity x(t) but a
// first-order low-pass of it, tau*y' = x - y with tau = 100 ms
// (profiles/busy_counter_calibration.txt: under a step to 100 % busy
// the reading goes 18, 33, 45, 55, 63 ... at 20 ms spacing, i.e.
// 1 - exp(-t/100)). Summing y*dt spreads a burst over the following
// few hundred ms — past the end of the lease that ran it, so a bursty
// pod would be under-charged. The filter inverts exactly:
//   integral of x over a step = integral of y + tau * (y_end - y_start)
// so each step is credited its own activity. The percent is an
// integer, which makes a single step uncertain by tau * 1 % = 1 ms;
// the tau term telescopes, so that error never adds up. A negative
// remainder (a rounding step down while idle) is carried into the
// next step instead of being dropped, for the same reason, and so is
// what a step's estimate exceeds its own length by. Rounding accounts
// for a carry of a ms or two either way. More than kMaxCarryMs means
// the reading is not smoothed the way this class assumes (a 100 ms
// filter cannot rise ten points within one 5 ms step):
// the excess is dropped, on both sides alike, rather than drained over
// later steps into leases that did not earn it.
class BusyPercentIntegrator {
 public:
  static constexpr double kTauMs = 100.0;
  static constexpr double kMaxCarryMs = 5.0;

  void reset(double pct) {
    last_pct_ = pct;
    carry_ms_ = 0.0;
  }

  // `pct` read now, `dt_ms` after the previous read. Returns the busy
  // ms of that interval, within [0, dt_ms].
  double step(double pct, double dt_ms) {
    if (dt_ms <= 0.0) return 0.0;
    pct = std::min(pct, 100.0);
    carry_ms_ += 0.5 * (pct + last_pct_) / 100.0 * dt_ms +
                 kTauMs * (pct - last_pct_) / 100.0;
    last_pct_ = pct;
    double busy = std::max(0.0, std::min(carry_ms_, dt_ms));
    carry_ms_ -= busy;
    carry_ms_ = std::max(-kMaxCarryMs, std::min(carry_ms_, kMaxCarryMs));
    return busy;
  }

 private:
  double last_pct_ = 0.0;
  double carry_ms_ = 0.0;
};

class BusySampler {
 public:
  // rsmi_utilization_counter_t: { RSMI_UTILIZATION_COUNTER_TYPE type;
  // uint64_t value; } — enum + padding puts value at offset 8.
  struct UtilCounter {
    int32_t type;      // 0 = RSMI_COARSE_GRAIN_GFX_ACTIVITY
    int32_t pad_;
    uint64_t value;
  };
  static_assert(sizeof(UtilCounter) == 16, "rsmi ABI");

  // device_index: rocm-smi enumeration order (the launcher passes the
  // same index it used for ROCR_VISIBLE_DEVICES / the sched port).
  bool init(int device_index) {
    dev_ = (uint32_t)device_index;
    lib_ = dlopen("librocm_smi64.so.7", RTLD_NOW | RTLD_LOCAL);
    if (!lib_) lib_ = dlopen("librocm_smi64.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib_) return false;
    auto init_fn = (int (*)(uint64_t))dlsym(lib_, "rsmi_init");
    if (!init_fn || init_fn(0) != 0) return false;
    // Preferred: the accumulating coarse-grain GFX activity counter —
    // "every millisecond the firmware calculates % busy and accumulates
    // it" (rocm_smi.h) — so busy_ms over any interval = delta/100,
    // exact even for sub-sampling-window bursts. Fallback: the busy
    // percent, through BusyPercentIntegrator.
    count_get_ = (int (*)(uint32_t, UtilCounter*, uint32_t, uint64_t*))
        dlsym(lib_, "rsmi_utilization_count_get");
    if (count_get_ && !counter_is_live()) count_get_ = nullptr;
    busy_get_ = (int (*)(uint32_t, uint32_t*))
        dlsym(lib_, "rsmi_dev_busy_percent_get");
    if (!count_get_) {
      uint32_t pct = 0;
      if (!busy_get_ || busy_get_(dev_, &pct) != 0) {
        busy_get_ = nullptr;
        return false;
      }
      from_pct_.reset((double)pct);
    }
    last_t_ = now_ms();
    return true;
  }

  bool active() const { return count_get_ != nullptr || busy_get_ != nullptr; }
  bool accumulating() const { return count_get_ != nullptr; }

  // Busy milliseconds since the previous poll.
  double poll() {
    if (count_get_) {
      UtilCounter c{0, 0, 0};
      uint64_t ts = 0;
      if (count_get_(dev_, &c, 1, &ts) == 0 && c.value >= last_acc_) {
        double busy = (double)(c.value - last_acc_) / 100.0;
        last_acc_ = c.value;
        return busy;
      }
      return 0.0;
    }
    if (!busy_get_) return 0.0;
    double now = now_ms();
    double dt = now - last_t_;
    last_t_ = now;
    uint32_t pct = 0;
    if (busy_get_(dev_, &pct) != 0) return 0.0;
    return from_pct_.step((double)pct, dt);
  }

 private:
  // The accumulating counter attributes busy time to a lease only if
  // the driver refreshes it about as often as gpu-schd polls. A
  // virtual function's driver publishes the metrics table once a
  // second: the total stays exact, but it arrives in one lump that
  // lands on whoever holds the token then, or on nobody. The table's
  // own timestamp (ns) tells the two apart: read it twice, 20 ms
  // apart, and require that it moved by about that much. A library
  // that reports no timestamp (0) therefore gets the percent path too.
  // Decided once, in init(), which it delays by those 20 ms, and never
  // revisited: a driver does not change its refresh rate under a
  // running gpu-schd. The log line at start names the source chosen.
  bool counter_is_live() {
    UtilCounter c{0, 0, 0};
    uint64_t ts0 = 0, ts1 = 0;
    if (count_get_(dev_, &c, 1, &ts0) != 0) return false;
    double t0 = now_ms();
    usleep(20 * 1000);
    if (count_get_(dev_, &c, 1, &ts1) != 0) return false;
    double wall = now_ms() - t0;
    double moved = (double)(int64_t)(ts1 - ts0) / 1e6;
    if (moved <= 0.0 || moved > 4.0 * wall) return false;
    last_acc_ = c.value;
    return true;
  }

  void* lib_ = nullptr;
  uint32_t dev_ = 0;
  double last_t_ = 0.0;
  uint64_t last_acc_ = 0;
  BusyPercentIntegrator from_pct_;
  int (*busy_get_)(uint32_t, uint32_t*) = nullptr;
  int (*count_get_)(uint32_t, UtilCounter*, uint32_t, uint64_t*) = nullptr;
};

}  // namespace ks
