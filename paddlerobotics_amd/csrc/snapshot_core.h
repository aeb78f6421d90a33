// snapshot_core.h -- the table that maps a robot's record (include/etgsim_snapshot.h) onto the simulator's arrays.
//
// Every persistent per-robot array is a SEGMENT of 4-byte words [rows][per * N] in which robot e owns the `per` consecutive
// columns per * e .. per * e + per - 1 of every row: per = 1 for the per-robot arrays (base, ctl, ...), per = 4 for the per-leg
// ones (column 4 e + leg), and the robot-major dynamic_param rows [N][48] are one row with per = 48.  Flag arrays of one byte
// per robot are widened to a word in the record.  In a record the segment's words follow each other row by row from word `off`.
// The lane mappings share the arrays' layout, so the table -- and a record -- is the same for both.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace etg {
namespace snapshot {

constexpr int kMaxSegs = 24;
constexpr int kHeadWords = 4;   // a record starts with 16 bytes: word 0 = the robot id it was saved from, the rest zero

struct Seg {
  void* p;       // the array, or null: not allocated (saved as zeros, skipped by a restore)
  int off;       // first word of the segment in a record
  int rows, per;
  int bytes;     // 1: the array holds one byte per robot (rows = per = 1)
};

struct Table {
  Seg seg[kMaxSegs];
  int nseg;
  int row_words;   // words per record, a multiple of 4
  int n_env;
};

}  // namespace snapshot
}  // namespace etg

// gather (write = 0: arrays -> records) or scatter (write = 1: records -> arrays) of n records; ids: the robot of each record,
// or null: record i is robot i.  The caller has checked the ids.
hipError_t etg_snapshot_launch(const etg::snapshot::Table& T, const int32_t* ids, int n, uint32_t* rows, int write, hipStream_t stream);
