// ricepp_stats.h -- loop trip counters and phase timers of the diagnostic
// build (-DRPP_STATS); nothing in a normal build.  A kernel that uses them
// declares `uint32_t stat_acc[16]` and `unsigned long long tprev_`, and adds
// stat_acc to its translation unit's own counter array at the end (a
// __device__ array cannot span translation units without relocatable device
// code): rpp_enc_stats_fetch and rpp_dec_stats_fetch read the two arrays.
#pragma once

#ifdef RPP_STATS
#define RPP_STAT(i, v) (stat_acc[i] += (v))
// phase timer: adds the s_memtime delta since the previous stamp to slot i
#define RPP_TSTAMP(i)                                                   \
  do {                                                                  \
    unsigned long long now_;                                            \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_)::"memory"); \
    stat_acc[i] += (uint32_t)(now_ - tprev_);                            \
    tprev_ = now_;                                                      \
  } while (0)
#else
#define RPP_STAT(i, v) ((void)0)
#define RPP_TSTAMP(i) ((void)0)
#endif
