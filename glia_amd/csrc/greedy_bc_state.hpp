// glia_amd/csrc/greedy_bc_state.hpp -- what the classifier loop's set-up and host driver (greedy_bc_setup.hip, compiled once) share
// with the instances of its kernels (greedy_bc.hip, compiled once per instance: hmt_internal.hpp): the state the kernels take as
// their argument, the sizes of the arrays the driver allocates for them, and the few calls the driver makes into an instance.
#pragma once
#include "bc_features.hpp"
#include "forest.hpp"
#include "greedy_common.hpp"

namespace glia {

#ifndef GLIA_BC_THREADS
#define GLIA_BC_THREADS 512
#endif
constexpr int kBcThreads = GLIA_BC_THREADS;   // 512: 256 VGPRs per thread (1024 spilled into scratch, measured 8% slower); >= 512 needed: the feature blocks of a 96-record chunk take 8 waves

constexpr uint32_t kJobMax = 1u << 14;    // records per job = slots of the votes array and rows of hrec; a contraction with more scores locally
constexpr uint32_t kRowWords = 32;        // 8-byte words of a record's row in hrec
constexpr uint32_t kFlagReps = 16, kFlagStride = 64;     // copies of the job flag, 256 bytes apart: 255 pollers on ONE word queue up at its memory channel
constexpr uint32_t kJobBufs = 4;          // job descriptors in flight (slot = sequence % kJobBufs; see bc_helper_loop)
constexpr uint32_t kJobWords = 4;          // ne0 | cnt << 32, r2 | newcount << 32, sequence, -
constexpr uint32_t kJob2Words = 1 + 5 * kMaxChannels;

// statistics of one image channel (a distinct volume + histogram among the feature lists); channel 0 = boundary
// probability: its counts and thresholded counts also serve the shape features
struct BcChan {
  // regions [2*R0]
  PStats* pts;
  EStats* Bn;          // non-mutual out-entries of the region's leaves
  EStats* Bt;          // additive totals of the whole boundary set (min/max fields unused)
  float* Bmn; float* Bmx;   // min / max over the whole boundary set
  // histogram entropies of pts[r] and Bt[r] (both fixed for the lifetime of region r): the leaf kernel files them for the
  // leaves, the scoring pass of the contraction that creates r for merged regions; a record's neighbour-side entropies are
  // then two loads instead of two passes over the bins (a division and a logarithm per bin)
  double* entP; double* entB;
  // records [Ecap]
  EStats* e_A;         // mutual entries, both directions
  EStats* e_NA;        // always-alive non-mutual entries, both directions
  float* e_dir;        // [Ecap][4]  mutual u->v min,max ; v->u min,max
  float2* pool_dir;    // [pool_cap] parallel to the incident lists: (min, max) the list's owner sends along that entry's
                       // record, (+inf, -inf) for dead entries -- the "all but one record" scans read it contiguously
  // leaf entries [P]
  EStats* le_stats;
};

// The same in every instance.  The instance with the MLP scorer appends its model to it in a type of its own (greedy_bc.hip).
struct BcState {
  uint32_t R0;
  BcChan ch[kMaxChannels];
  uint32_t* parent;    // merge forest (find -> current region of a leaf)
  uint32_t* adj_off; uint32_t* adj_len; uint32_t* pool; unsigned long long pool_cap;
  // records [Ecap]
  uint32_t Ecap;
  uint32_t *e_u, *e_v, *e_posu, *e_posv;
  uint8_t *e_alive, *e_table, *e_orient;    // orient: 1 = features take (u, v), 0 = (v, u)
  uint32_t *e_fhead, *e_ftail;   // fragile non-mutual leaf entries (linked through le_next), kNone = empty
  PqTree pq;
  // leaf entries [P] (directed label pairs, ascending (a,b))
  long long P;
  uint32_t *le_src, *le_dst;     // dense leaf ids
  uint32_t* le_next;
  uint8_t* le_mutual;
  uint32_t* le_start;            // [R0+1] first out-entry of each leaf
  uint32_t* nm_out;              // [R0] non-mutual out-entries per leaf
  uint32_t *mark0, *mark1;       // [2*R0]
  uint32_t* order; double* sal_out; double* feats_out;
  // Helper workgroups score WHOLE records (round 3): the loop's workgroup publishes a job -- "records ne0 .. ne0 + cnt of the region
  // r2 just created" -- and helper h takes the records h, h + H, ...: it stages everything a record's vector needs with agent-scope
  // loads, computes neighbour extremes, shared-boundary set, entropies, the vector and the forest's votes, and answers with one
  // 64-bit word per record.  Everything a helper reads that this launch writes is stored write-through (st_agent) by the loop.
  // What the loop's workgroup re-reads itself (the records' own fields and statistics, list headers) it keeps in plain stores --
  // a write-through store drops the line from its XCD's L2 and every later read of it went to memory (measured: +10 k cycles
  // per contraction) -- and hands the helpers a COPY: one packed 256-byte row per new record and channel (hrec), hadj for the
  // list headers.  Region statistics, set extremes, entropies, pool_dir and the merge forest are stored write-through only.
  uint32_t* hctl;                // [kFlagReps * kFlagStride] job sequence number (never 0; 0xFFFFFFFF = quit), replicated: helper h polls copy h % kFlagReps
  unsigned long long* hjob;      // [kJobBufs][kJobWords] job descriptors, slot = sequence % kJobBufs
  // Round 4: a job goes out in TWO parts.  Part 1 (hjob + hctl) as soon as the contraction's records are built -- the helpers stage
  // rows and region statistics, form the shared sets and the entropies (S0-S3) while the loop's workgroup is still finding the top two
  // of r2's extremes; part 2 (hjob2 + hctl2: those extremes and min / max of B(r2)) is what the vector assembly (S4) waits for.
  uint32_t* hctl2;               // [kFlagReps * kFlagStride] sequence number of the newest job whose part 2 is out
  unsigned long long* hjob2;     // [kJobBufs][kJob2Words] sequence | per channel: best_mn, best_mx, second_mn, second_mx, (Bmn | Bmx << 32) of r2
  unsigned long long* hvotes;    // [kJobMax] sequence << 32 | model << 24 | votes, indexed by the record's position in the job
  unsigned long long* hrec;      // [kJobMax][K][kRowWords] rows of the current job: e_A | e_NA | rs, own slot | table flag, fragile head
  unsigned long long* hadj;      // [2*R0] adj_off | adj_len << 32 for the helpers
  uint32_t n_helpers;            // workgroups 1..n_helpers score records; 0 = the loop's own workgroup does
  uint32_t shard, n_shards;      // initial scoring: this call scores the records e with e % n_shards == shard (multi-GPU K7)
  unsigned long long* ctrl;
  unsigned long long max_iters;
  const uint32_t* forced;        // bc_feat mode: [forced_n][2] region pairs to merge, in this order (no queue, no scoring)
  unsigned long long forced_n;
  BcCfg cfg;
  DeviceClassifier clf;
};

// What the driver asks of an instance: its three kernels on the driver's state (req: the MLP instance takes its model from it), and
// how many workgroups of its loop kernel one compute unit holds.  One constant of this type per instance, behind the accessors of
// hmt_internal.hpp.
struct BcInstance {
  bool has_mlp;                  // holds the MLP scorer (DeviceClassifier::kind == 2)
  void (*init_score)(const BcState& st, const BcRequest& req, uint32_t E0, hipStream_t stream);
  void (*init_score_median)(const BcState& st, const BcRequest& req, uint32_t e0, uint32_t e1, const double* reg, const double* bnd, hipStream_t stream);
  void (*loop)(const BcState& st, const BcRequest& req, hipStream_t stream);        // on 1 + st.n_helpers workgroups
  hipError_t (*loop_workgroups_per_cu)(int* per_cu);
};

}  // namespace glia
