// fleet_train.h -- constants of PPO's whole update on the device (fleet_train.hip): the keyed shuffle's shape and the launch shapes
// of the minibatch launch and of the closing reduction.  tests/train_model.py restates them.
#pragma once
#include <stdint.h>

#include "../../include/fleet_hip.h"

// perm(n, seed, epoch, p): a balanced Feistel network over 2h bits, h the smallest h >= kTrainMinHalfBits with 2^(2h) >= n, of
// kTrainRounds rounds, cycle-walked into [0, n).  Eight rounds on a domain of at least 256 values pass the uniformity condition of
// tests/test_ppo_train_cpu.py at n = 5, 15 and 40 (four rounds on the smallest domain fail it by a factor of eight).
constexpr int kTrainRounds = 8;
constexpr int kTrainMinHalfBits = 4;
// train_minibatch / train_finish: 256 threads = 4 wavefronts; an ordered sum is 256 lane sums and a halving tree over them.
constexpr int kTrainThreads = 256;
// train_minibatch: a tile is kTrainRows consecutive rows of the minibatch, one per wavefront (a row after another is a chain of
// memory latencies: 16 rows per workgroup cost four of them); a workgroup strides
// over the tiles, at most kTrainMaxBlocks workgroups per launch; the buffer rows of the first kTrainCache positions of the minibatch
// are kept in the LDS (positions behind them are evaluated again where they are needed).
constexpr int kTrainRows = 4;
constexpr int kTrainMaxBlocks = 256;
constexpr int kTrainCache = 2048;
static_assert(kTrainThreads == 256 && kTrainRows % (kTrainThreads / 64) == 0, "whole wavefronts, the same number of rows each");
static_assert(kTrainCache % kTrainThreads == 0, "the cached positions are whole passes of the workgroup");
static_assert(FLEET_TRAIN_ROUNDS == kTrainRounds && FLEET_TRAIN_MIN_HALF_BITS == kTrainMinHalfBits, "the header states the shuffle");
