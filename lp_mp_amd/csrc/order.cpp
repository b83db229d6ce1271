// order.cpp — see plan.hpp.  The ticket orders of the Infinity-Cache chain launches: what the joined passes of a three-step
// pass depend on (plan_rotation_chain), their window (rot_geometry), the skewed band order, the tiled order, and the tables of
// one joined-pass launch.  Host only (no HIP): engine.cpp caches, uploads and launches what is built here.
#include "plan.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <stdexcept>

namespace lpmp {

namespace {

// who touches what in one launch: the block (of gpb records) whose record updates factor g or reaches it through an op
std::vector<int32_t> launch_touchers(const Schedule& s, const LevelRange& lr, int gpb, int64_t nf) {
  std::vector<int32_t> t((size_t)nf, -1);
  for (int64_t i = lr.begin; i < lr.end; ++i) {
    const UpdRec& r = s.recs[i];
    const int32_t b = (int32_t)((i - lr.begin) / gpb);
    t[r.factor] = b;
    for (int k = 0; k < r.n_recv + r.n_send; ++k) t[s.ops[r.op_begin + k].peer] = b;
  }
  return t;
}

// Peer minima (kernels.hip, dense_pq_*_body): may the W records publish, per edge, what the record at the other end computes
// from the table?  "" or the first obstacle.  The W step: every record receives and then sends over the same <= 4 edges, each
// send forwarding a distinct receive (Op::pad of the send = index of the receive + 1, and the receive is marked deferred).  The
// H, K, T steps: at most 4 receives and 4 sends, H receives nothing (no slot is written before it), and every receive of K and T
// reads a pairwise factor that exactly one W record receives-and-sends.
std::string peer_minima_obstacle(const Schedule& fb, const Schedule& bf, const LevelRange& h, const LevelRange& w, const LevelRange& k,
                                 const LevelRange& t, int64_t nf) {
  if (w.kclass != KC_DENSE_32) return "not the exact 32-label dense class";
  for (const LevelRange* lr : {&h, &w, &k, &t}) if (lr->stride <= 0 || lr->stride > 1 + PK_MAX_OPS) return "a step is not in packet form";
  std::vector<uint8_t> pub((size_t)nf, 0);
  for (int64_t i = w.begin; i < w.end; ++i) {
    const UpdRec& r = fb.recs[i];
    if (r.n_recv != r.n_send || r.n_recv > PEER_MINIMA_MAX_OPS) return "a W record does not send over exactly the <= 4 edges it receives from";
    uint32_t seen = 0;
    for (int q = 0; q < r.n_send; ++q) {
      const Op& o = fb.ops[r.op_begin + r.n_recv + q];
      if (o.pad < 1 || o.pad > r.n_recv || ((seen >> o.pad) & 1u)) return "a W send does not forward a receive of its own";
      seen |= 1u << o.pad;
      if (fb.ops[r.op_begin + o.pad - 1].peer != o.peer) return "a W send forwards a receive of another factor";
    }
    for (int q = 0; q < r.n_recv; ++q) {
      const Op& o = fb.ops[r.op_begin + q];
      if (o.pad == 0) return "a W receive is stored before its send";
      if (o.peer < 0 || o.peer >= nf || pub[o.peer]) return "two W records reach one pairwise factor";
      pub[o.peer] = 1;
    }
  }
  for (int64_t i = h.begin; i < h.end; ++i) {
    const UpdRec& r = fb.recs[i];
    if (r.n_recv != 0 || r.n_send > PEER_MINIMA_MAX_OPS) return "an H record receives, or sends over more than 4 edges";
  }
  for (int which = 0; which < 2; ++which) {
    const Schedule& s = which == 0 ? bf : fb;
    const LevelRange& lr = which == 0 ? k : t;
    for (int64_t i = lr.begin; i < lr.end; ++i) {
      const UpdRec& r = s.recs[i];
      if (r.n_recv > PEER_MINIMA_MAX_OPS || r.n_send > PEER_MINIMA_MAX_OPS) return "a K / T record has more than 4 receives or sends";
      for (int q = 0; q < r.n_recv; ++q) {
        const int32_t f = s.ops[r.op_begin + q].peer;
        if (f < 0 || f >= nf || !pub[f]) return "a K / T receive reads a pairwise factor no W record receives-and-sends";
      }
    }
  }
  return "";
}

}  // namespace

RotationInfo plan_rotation_chain(const Schedule& fb, const Schedule& bf, int64_t nf, int consume_gpb) {
  RotationInfo ri;
  auto only_launch = [](const Schedule& s, int level, LevelRange& out) {
    int n = 0;
    for (const auto& lr : s.launches) if (lr.level == level) { out = lr; ++n; }
    return n == 1;
  };
  LevelRange h, w, k, t;
  if (!only_launch(fb, 1, h) || !only_launch(fb, 2, w) || !only_launch(fb, 3, t) || !only_launch(bf, 2, k)) return ri;
  const int kc = w.kclass;
  if (h.kclass != kc || k.kclass != kc || t.kclass != kc || !kc_is_packed(kc)) return ri;
  ri.kclass = kc; ri.gpb = kc_block_records(kc);
  ri.consume_gpb = consume_gpb > 0 ? consume_gpb : ri.gpb;
  const int tg[4] = {ri.consume_gpb, ri.gpb, ri.consume_gpb, ri.consume_gpb};   // records per block of H, W, K, T
  const LevelRange* lrs[4] = {&h, &w, &k, &t};
  const Schedule* sch[4] = {&fb, &fb, &bf, &fb};
  std::vector<int32_t> touch[4];
  for (int i = 0; i < 4; ++i) {
    const int64_t cnt = lrs[i]->end - lrs[i]->begin;
    ri.t[i] = {i == 2 ? 1 : 0, *lrs[i], (int32_t)((cnt + tg[i] - 1) / tg[i]), cnt, lrs[i]->n_recv, lrs[i]->bytes};
    touch[i] = launch_touchers(*sch[i], *lrs[i], tg[i], nf);
  }
  // kind -> (X, Y1, Y2)
  const int X[6] = {1, 2, 1, 2, 3, 3}, Y1[6] = {0, 1, 2, 1, 1, 1}, Y2[6] = {-1, 0, 1, 2, 2, 0};
  for (int kind = 0; kind < 6; ++kind) {
    const Schedule& s = *sch[X[kind]];
    const LevelRange& lr = *lrs[X[kind]];
    // (blocks are independent: chunks of them on several threads, see plan.hpp parallel_blocks)
    const int64_t nbk = ri.t[X[kind]].nb, gx = tg[X[kind]];
    std::vector<std::vector<std::pair<int8_t, int32_t>>> per((size_t)nbk);
    parallel_blocks(nbk, 4096, [&](int64_t b0, int64_t b1) {
      for (int64_t b = b0; b < b1; ++b) {
        auto& dst = per[(size_t)b];
        for (int64_t i = lr.begin + b * gx; i < std::min<int64_t>(lr.end, lr.begin + (b + 1) * gx); ++i) {
          const UpdRec& r = s.recs[i];
          auto visit = [&](int32_t g) {
            if (touch[Y1[kind]][g] >= 0) dst.emplace_back((int8_t)1, touch[Y1[kind]][g]);
            else if (Y2[kind] >= 0 && touch[Y2[kind]][g] >= 0) dst.emplace_back((int8_t)2, touch[Y2[kind]][g]);
          };
          visit(r.factor);
          for (int q = 0; q < r.n_recv + r.n_send; ++q) visit(s.ops[r.op_begin + q].peer);
        }
        std::sort(dst.begin(), dst.end());
        dst.erase(std::unique(dst.begin(), dst.end()), dst.end());
      }
    });
    ri.off[kind].assign(1, 0);
    for (auto& v : per) {
      for (const auto& d : v) { ri.delta[kind].push_back(d.first); ri.block[kind].push_back(d.second); }
      ri.off[kind].push_back((int64_t)ri.block[kind].size());
    }
    if (kind == 2 || kind == 3) {
      const double nbs = (double)std::max<int64_t>(1, nbk), nbp = (double)std::max<int32_t>(1, ri.t[Y1[kind]].nb);
      for (int64_t b = 0; b < nbk; ++b)
        for (const auto& d : per[(size_t)b])
          if (d.first == 1) ri.reach = std::max(ri.reach, (d.second + 0.5) / nbp - (b + 0.5) / nbs);
    }
  }
  {   // coverage of the per-pass bound rows (kernels.hpp HIST_END / HIST_MID)
    std::vector<uint8_t> cov((size_t)nf, 0);
    for (int64_t i = w.begin; i < w.end; ++i) cov[fb.recs[i].factor] = 1;
    for (int64_t i = k.begin; i < k.end; ++i) {
      const UpdRec& r = bf.recs[i];
      cov[r.factor] = 1;
      for (int q = 0; q < r.n_recv; ++q) cov[bf.ops[r.op_begin + q].peer] = 1;
    }
    ri.hist_ok = true;
    for (int64_t f = 0; f < nf; ++f) if (!cov[f]) { ri.hist_ok = false; break; }
  }
  ri.peer_minima_why = peer_minima_obstacle(fb, bf, h, w, k, t, nf);
  ri.peer_minima = ri.peer_minima_why.empty();
  ri.valid = true;
  return ri;
}

// The window of the skewed order — (bands, lag, depth) — from the model (round 6).  A table is read by two consecutive steps; with
// bands of a step issued at time b + lag * d (d = the step's place in its group of `depth` steps) the second read comes
// lag * depth bands after the first, and it finds the table in the 256 MiB Infinity Cache while that window stays below it.
// The lag has to cover the REACH of the dependencies — how far ahead in the block list a block's predecessors lie: one grid row —
// plus slack: a ticket whose predecessors were issued fewer tickets ago than there are resident workgroups (256 CUs x 3) is drawn
// while they are still running, and its workgroup waits.  In ticket order the steps of a group are interleaved, so a slack of
// S tickets is S / depth blocks of one step.  Measured (profiles/r06_blocked_pass_probe_*.txt, 32 labels, bands of 16 MiB, a
// block = 156 KB): 1024^2 (row 20 MB) lag 3, depth 4: 5.12 ms per pass (lag 2: 5.24, lag 4: 5.18); 1536^2 (row 30 MB) lag 3 / 4 / 5:
// 12.17 / 11.94 / 12.85 (11.5 = 2.25 times the 1024^2 time; 14.5 launch by launch); 2048^2 (row 40 MB) 25.3 with lag 3 (slack
// 260 tickets: no better than one launch per step, 26.0), 21.3 with lag 4 (700 tickets; 20.4 = four times), 22.6 with lag 5
// (window 336 MB: the reuse goes); 3072^2 (row 60 MB) 65.4 with lag 3 / depth 4 (57.2 launch by launch), 50.3 with lag 6 / depth 2
// (46 = nine times; depth 3 and 4 with lags 5-6: 50.2-52.1).  So: a slack of 700 tickets behind the reach; depth 4 while
// (reach + slack) * 4 stays under 275 MiB, else 2 (half of the second reads instead of three quarters, but they hit); the lag
// stretched to a window of 200 MiB where the reach leaves room; `fits` = false when even depth 2 cannot hold the window (then the
// tiled order below, or one launch per step).
RotGeometry rot_geometry(const RotSettings& rs, const RotationInfo& ri) {
  RotGeometry g;
  g.lag = std::max(1, rs.lag); g.depth = std::max(1, rs.depth);
  if (!ri.valid || ri.t[1].bytes <= 0 || ri.t[1].nb <= 0) return g;   // (no step to measure: the defaults)
  g.bands = rs.bands > 0 ? rs.bands : (int)std::max<int64_t>(1, std::min<int64_t>(ri.t[1].nb, ri.t[1].bytes / ((int64_t)16 << 20)));
  if (rs.bands > 0) return g;                       // bands forced (tests, probes): lag and depth as given or their defaults
  constexpr double MiB = 1048576.0, SLACK_TICKETS = 700, WINDOW_TARGET = 200 * MiB, WINDOW_MAX = 275 * MiB;
  const double step_bytes = (double)ri.t[1].bytes, band_bytes = step_bytes / g.bands;
  const double slack1 = SLACK_TICKETS * step_bytes / (double)ri.t[1].nb;   // the slack as bytes of ONE step's block list, depth 1
  g.reach_bytes = ri.reach * step_bytes;
  if (!rs.depth_set) g.depth = (g.reach_bytes + slack1 / 4) * 4 <= WINDOW_MAX ? 4 : 2;
  const double need = g.reach_bytes + slack1 / g.depth;
  // (rounded up from .3: a band short on slack costs more than a band of window — 1536^2: 3.4 bands -> 4)
  if (!rs.lag_set) g.lag = std::max(2, (int)std::floor(std::max(need, WINDOW_TARGET / g.depth) / band_bytes + 0.7));
  g.fits = rs.depth_set || rs.lag_set || need * g.depth <= 1.25 * WINDOW_MAX;
  return g;
}

// Tiled ticket order (round 6; chosen in engine.cpp rotation_chain, LPMP_ROT_TILES overrides).  The band order walks a step's block
// list in memory order, so its lag has to cover how far ahead a block's predecessors lie IN THAT LIST — a grid row, a z-slice of a
// 3-D grid — whatever the distance in the graph is.  Tiles are compact in the GRAPH instead: sets of about T blocks of either
// alternating step template (W and K; H and T update K's factors), grown breadth-first over the block dependencies.  Inside a group
// of `depth` steps a block runs in the phase of its own tile or of the latest tile one of its predecessors ran in, whichever is
// later — the skew of a time-tiled stencil without any geometry: valid by construction, a table is read again by the next step T
// blocks later, and nothing grows with the width of the grid.
namespace {

int32_t grow_tiles(const RotationInfo& ri, int64_t T, std::vector<int32_t>& tile_w, std::vector<int32_t>& tile_k, double& radius) {
  const int64_t nw = ri.t[1].nb, nk = ri.t[2].nb, nn = nw + nk;
  std::vector<int64_t> deg((size_t)nn + 1, 0);
  auto each_edge = [&](auto f) {      // W block j <-> K block p (kind 2: W after K), K block j <-> W block p (kind 3: K after W)
    for (int kind = 2; kind <= 3; ++kind) {
      const int64_t nb = kind == 2 ? nw : nk;
      for (int64_t j = 0; j < nb; ++j)
        for (int64_t q = ri.off[kind][j]; q < ri.off[kind][j + 1]; ++q)
          if (ri.delta[kind][q] == 1) { const int64_t a = kind == 2 ? j : nw + j, b = kind == 2 ? nw + ri.block[kind][q] : ri.block[kind][q]; f(a, b); }
    }
  };
  each_edge([&](int64_t a, int64_t b) { ++deg[a + 1]; ++deg[b + 1]; });
  for (int64_t i = 0; i < nn; ++i) deg[i + 1] += deg[i];
  std::vector<int32_t> adj((size_t)deg[nn]);
  { std::vector<int64_t> cur(deg.begin(), deg.end() - 1); each_edge([&](int64_t a, int64_t b) { adj[cur[a]++] = (int32_t)b; adj[cur[b]++] = (int32_t)a; }); }
  std::vector<int32_t> tile((size_t)nn, -1), queue, hops;
  int32_t n_tiles = 0;
  double radius_sum = 0; int64_t full_tiles = 0;    // hops from the seed to the last block of a tile that reached its size
  for (int64_t seed0 = 0; seed0 < std::max(nw, nk); ++seed0)
    for (int64_t seed : {seed0 < nw ? seed0 : (int64_t)-1, seed0 < nk ? nw + seed0 : (int64_t)-1}) {
      if (seed < 0 || tile[seed] >= 0) continue;
      queue.assign(1, (int32_t)seed); hops.assign(1, 0);
      int64_t taken = 0; int32_t last_hops = 0;
      for (size_t head = 0; head < queue.size() && taken < 2 * T; ++head) {
        const int32_t v = queue[head];
        if (tile[v] >= 0) continue;
        tile[v] = n_tiles; ++taken; last_hops = hops[head];
        for (int64_t q = deg[v]; q < deg[v + 1]; ++q) if (tile[adj[q]] < 0) { queue.push_back(adj[q]); hops.push_back(hops[head] + 1); }
      }
      if (taken >= 2 * T) { radius_sum += last_hops; ++full_tiles; }
      ++n_tiles;
    }
  radius = full_tiles ? radius_sum / (double)full_tiles : 0.0;
  tile_w.assign(tile.begin(), tile.begin() + nw);
  tile_k.assign(tile.begin() + nw, tile.end());
  return n_tiles;
}

// how much of a tile is left after sd steps: phases of a steady-state group (K, W, K, W, ...) of n_steps steps, share of delayed blocks per step
void tile_delays(const RotationInfo& ri, const std::vector<int32_t>& tile_w, const std::vector<int32_t>& tile_k, double (&delayed)[TILE_STEPS_MAX], int n_steps) {
  std::vector<int32_t> ph[3];
  for (int sd = 0; sd < n_steps; ++sd) {
    const int kd = sd % 2 == 0 ? 3 : 2;
    const std::vector<int32_t>& tl = sd % 2 == 0 ? tile_k : tile_w;
    const int64_t nb = (int64_t)tl.size();
    std::vector<int32_t>& cur = ph[sd % 3];
    cur.resize((size_t)nb);
    int64_t late = 0;
    for (int64_t j = 0; j < nb; ++j) {
      int32_t p = tl[j];
      if (sd > 0)
        for (int64_t q = ri.off[kd][j]; q < ri.off[kd][j + 1]; ++q) {
          const int dl = ri.delta[kd][q];
          if (dl <= sd) p = std::max(p, ph[(sd - dl) % 3][ri.block[kd][q]]);
        }
      cur[j] = p;
      late += p != tl[j];
    }
    delayed[sd] = nb ? (double)late / (double)nb : 0.0;
  }
}

// the 2 n + 1 steps of n joined passes — H, W, (K, W)^(n-1), T — as templates (0 H, 1 W, 2 K, 3 T) and the kind of their
// predecessor lists in RotationInfo (-1: none)
void joined_steps(int n, std::vector<int>& tmpl, std::vector<int>& kind) {
  const int n_steps = 2 * n + 1;
  tmpl.assign(n_steps, 0); kind.assign(n_steps, -1);
  for (int s = 1; s < n_steps - 1; ++s) tmpl[s] = (s & 1) ? 1 : 2;
  tmpl[n_steps - 1] = 3;
  for (int s = 1; s < n_steps; ++s) kind[s] = s == n_steps - 1 ? (n == 1 ? 5 : 4) : s == 1 ? 0 : s == 2 ? 1 : (s & 1) ? 2 : 3;
}

}  // namespace

TileSet make_tiles(const RotationInfo& ri, int T) {
  TileSet ts;
  ts.T = T;
  ts.n = grow_tiles(ri, T, ts.w, ts.k, ts.radius);
  tile_delays(ri, ts.w, ts.k, ts.delayed, 8);
  // a block whose predecessor ran in a later tile is delayed to that tile's phase — one more shell of every tile per step: the
  // deepest even depth (up to 8) whose LAST step still runs at least half of its blocks in their own tile's phase
  ts.depth = 2;
  for (int d = 4; d <= 8; d += 2) if (ts.delayed[d - 1] <= 0.5) ts.depth = d;
  return ts;
}

void extend_tile_delays(const RotationInfo& ri, TileSet& ts) {
  if (ts.delays_extended || ts.T <= 0) return;
  tile_delays(ri, ts.w, ts.k, ts.delayed, TILE_STEPS_MAX);
  ts.delays_extended = true;
}

// Measured on 1024^2 x 32 labels (EXPERIMENTS.md T).  PQ_TILE_BYTES of a W step per tile is what 8192 blocks per tile are on that grid:
// such a tile is NOT inside the Infinity Cache, and is not meant to be — tiles only make the reach of the dependencies a row of a
// tile, large ones have few blocks on a rim, and the distance between two reads of a table comes from the lag alone (2 x PQ_SUB_LAG
// times of depth / 2 W sub-bands each, about 150 MB of tables).  4096 blocks were 1 % slower, 2048 3 %, 32768 5 %; nothing else between
// 4096 and 32768 was tried.  PQ_SUB_TICKETS W tickets per sub-band, PQ_SUB_LAG times between consecutive steps, PQ_SUB_GAP times at least
// behind every predecessor, groups of at most PQ_DEPTH steps (12 and 16 were slower).
namespace {
constexpr double PQ_TILE_BYTES = 1662.0 * 1048576.0;
constexpr int PQ_SUB_TICKETS = 64, PQ_SUB_LAG = 3, PQ_SUB_GAP = 2, PQ_DEPTH = 8;
constexpr int64_t PQ_TABLE_BYTES = 32 * 32 * 8, PQ_MINIMA_BYTES = 32 * 8, INFINITY_CACHE_BYTES = (int64_t)256 << 20;
}  // namespace

PqGeometry peer_minima_geometry(const RotationInfo& ri, int tile_blocks) {
  PqGeometry g;
  // (PQ_TABLE_BYTES / PQ_MINIMA_BYTES are the exact 32-label f64 class's, the only one peer_minima_obstacle admits)
  if (!ri.valid || !ri.peer_minima || ri.kclass != KC_DENSE_32 || ri.t[1].nb <= 0 || ri.t[2].nb <= 0) return g;
  for (int i = 0; i < 4; ++i)
    g.step_bytes[i] = i == 1 ? ri.t[i].bytes + ri.t[i].recv * PQ_MINIMA_BYTES : std::max<int64_t>(0, ri.t[i].bytes - ri.t[i].recv * (PQ_TABLE_BYTES - PQ_MINIMA_BYTES));
  g.use = ri.t[1].recv * PQ_TABLE_BYTES > INFINITY_CACHE_BYTES;
  const double nw = (double)ri.t[1].nb, nk = (double)ri.t[2].nb, w_block_bytes = (double)g.step_bytes[1] / nw;
  // a tile of T blocks holds about 2 T blocks of the W and K steps together (order.cpp grow_tiles), W and K in the ratio of their counts
  const double w_share = 2.0 * nw / (nw + nk);
  g.tile_blocks = tile_blocks > 0 ? tile_blocks : (int)std::max(1.0, std::min(nw, std::floor(PQ_TILE_BYTES / w_block_bytes / w_share + 0.5)));
  g.w_blocks_per_tile = std::min(nw, g.tile_blocks * w_share);
  g.tile_bytes = g.w_blocks_per_tile * w_block_bytes;
  g.sub = (int)std::max(1.0, std::floor(g.w_blocks_per_tile / PQ_SUB_TICKETS));
  g.sub_lag = PQ_SUB_LAG; g.sub_gap = PQ_SUB_GAP;
  g.depth = PQ_DEPTH;                      // (what make_tiles allows at most: the rule takes TileSet::depth)
  return g;
}

double peer_minima_hbm_share(const TileSet& ts, int depth) {
  if (depth < 2) return 1.0;
  double late = 0;
  for (int sd = 3; sd < std::min(depth, TILE_STEPS_MAX); sd += 2) late += ts.delayed[sd];
  return std::min(1.0, (1.0 + late) / (depth / 2));
}

void band_order(const std::vector<int64_t>& nb, int bands, int lag, int depth, TicketOrder& o) {
  const int n_steps = (int)nb.size();
  std::vector<int64_t> base((size_t)n_steps + 1, 0);
  for (int s = 0; s < n_steps; ++s) base[s + 1] = base[s] + nb[s];
  const int64_t N = base[n_steps];
  o.tk_step.resize((size_t)N); o.tk_block.resize((size_t)N); o.new_of.resize((size_t)N); o.group_begin.clear();
  auto band_begin = [](int64_t b, int64_t nbs, int64_t bands_) { return (b * nbs + bands_ - 1) / bands_; };   // first block of band b
  int64_t at = 0;
  for (int s0 = 0; s0 < n_steps; s0 += depth) {
    o.group_begin.push_back(at);
    const int d = std::min(depth, n_steps - s0);
    for (int64_t tau = 0; tau < bands + (int64_t)lag * (d - 1); ++tau)
      for (int sd = 0; sd < d; ++sd) {
        const int64_t b = tau - (int64_t)lag * sd;
        if (b < 0 || b >= bands) continue;
        const int s = s0 + sd;
        for (int64_t j = band_begin(b, nb[s], bands); j < band_begin(b + 1, nb[s], bands); ++j) {
          o.new_of[base[s] + j] = (int32_t)at; o.tk_step[at] = s; o.tk_block[at] = (int32_t)j; ++at;
        }
      }
  }
  o.group_begin.push_back(at);
}

void tiled_order(const RotationInfo& ri, int n, const TileSet& ts, int depth, TicketOrder& o) {
  std::vector<int> tmpl, kind;
  joined_steps(n, tmpl, kind);
  const int n_steps = (int)tmpl.size();
  std::vector<int64_t> base((size_t)n_steps + 1, 0);
  for (int s = 0; s < n_steps; ++s) base[s + 1] = base[s] + ri.t[tmpl[s]].nb;
  const int64_t N = base[n_steps];
  o.tk_step.resize((size_t)N); o.tk_block.resize((size_t)N); o.new_of.resize((size_t)N); o.group_begin.clear();
  // phase of (step of the group, block) = max(own tile, phases of its predecessors inside the group); tickets by (phase, step, block)
  std::vector<int32_t> ph[3];
  std::vector<int64_t> bucket;
  std::vector<std::vector<int32_t>> key_of((size_t)depth);
  int64_t at = 0;
  for (int s0 = 0; s0 < n_steps; s0 += depth) {
    o.group_begin.push_back(at);
    const int d = std::min(depth, n_steps - s0);
    bucket.assign((size_t)ts.n * d + 1, 0);
    for (int sd = 0; sd < d; ++sd) {
      const int s = s0 + sd;
      const int64_t nb = ri.t[tmpl[s]].nb;
      const std::vector<int32_t>& tl = tmpl[s] == 1 ? ts.w : ts.k;
      std::vector<int32_t>& cur = ph[sd % 3];
      cur.resize((size_t)nb);
      key_of[sd].resize((size_t)nb);
      const int kd = kind[s];
      for (int64_t j = 0; j < nb; ++j) {
        int32_t p = tl[j];
        if (kd >= 0)
          for (int64_t q = ri.off[kd][j]; q < ri.off[kd][j + 1]; ++q) {
            const int dl = ri.delta[kd][q];
            if (dl <= sd) p = std::max(p, ph[(sd - dl) % 3][ri.block[kd][q]]);
          }
        cur[j] = p;
        key_of[sd][j] = p * d + sd;
        ++bucket[(size_t)key_of[sd][j] + 1];
      }
    }
    for (size_t k = 0; k + 1 < bucket.size(); ++k) bucket[k + 1] += bucket[k];
    for (int sd = 0; sd < d; ++sd) {
      const int s = s0 + sd;
      const int64_t nb = ri.t[tmpl[s]].nb;
      for (int64_t j = 0; j < nb; ++j) {
        const int64_t t = at + bucket[key_of[sd][j]]++;
        o.new_of[base[s] + j] = (int32_t)t; o.tk_step[t] = s; o.tk_block[t] = (int32_t)j;
      }
    }
    for (int sd = 0; sd < d; ++sd) at += ri.t[tmpl[s0 + sd]].nb;
  }
  o.group_begin.push_back(at);
}

// Skewed tiled order (peer-minima launches; chosen in engine.cpp rotation_chain).  In the tiled order the steps of a phase run back to
// back, so the first tickets of every step are drawn while their predecessors still run, and a table is read again a whole tile
// later.  Here the blocks of a tile are cut, in block order, into `sub` sub-bands, the sub-bands of all tiles form one list in tile
// order, and sub-band b of the group's sd-th step comes at time b + lag * sd — the band order's skew over a list in which a block's
// predecessors lie a row of its TILE away, not a row of the grid.  Where they lie further (the rim of a tile next to a later one)
// the block waits for them: a block never comes before time(predecessor) + gap.  Valid by construction, whatever sub, lag and gap
// are.  Tickets by (time, step, block); sub <= 1 is tiled_order's order.
void skewed_tile_order(const RotationInfo& ri, int n, const TileSet& ts, int depth, int sub, int lag, int gap, TicketOrder& o) {
  if (sub <= 1) { tiled_order(ri, n, ts, depth, o); return; }
  std::vector<int> tmpl, kind;
  joined_steps(n, tmpl, kind);
  const int n_steps = (int)tmpl.size();
  std::vector<int64_t> base((size_t)n_steps + 1, 0);
  for (int s = 0; s < n_steps; ++s) base[s + 1] = base[s] + ri.t[tmpl[s]].nb;
  const int64_t N = base[n_steps];
  o.tk_step.resize((size_t)N); o.tk_block.resize((size_t)N); o.new_of.resize((size_t)N); o.group_begin.clear();
  lag = std::max(1, lag); gap = std::max(0, gap);
  if ((int64_t)ts.n * sub + (int64_t)(lag + gap) * depth >= INT32_MAX / (2 * depth)) throw std::runtime_error("rotation chain: too many sub-bands");
  // the sub-band of every W block and of every block of the other templates, counted through the tiles
  std::vector<int32_t> band[2];
  for (int which = 0; which < 2; ++which) {
    const std::vector<int32_t>& tl = which == 0 ? ts.w : ts.k;
    std::vector<int64_t> members((size_t)ts.n, 0), seen((size_t)ts.n, 0);
    for (int32_t t : tl) ++members[t];
    band[which].resize(tl.size());
    for (size_t j = 0; j < tl.size(); ++j) band[which][j] = (int32_t)((int64_t)tl[j] * sub + seen[tl[j]]++ * sub / members[tl[j]]);
  }
  std::vector<int32_t> tm[3];
  std::vector<int64_t> bucket;
  std::vector<std::vector<int32_t>> key_of((size_t)depth);
  int64_t at = 0;
  for (int s0 = 0; s0 < n_steps; s0 += depth) {
    o.group_begin.push_back(at);
    const int d = std::min(depth, n_steps - s0);
    int32_t t_max = 0;
    for (int sd = 0; sd < d; ++sd) {
      const int s = s0 + sd;
      const int64_t nb = ri.t[tmpl[s]].nb;
      const std::vector<int32_t>& bd = band[tmpl[s] == 1 ? 0 : 1];
      std::vector<int32_t>& cur = tm[sd % 3];
      cur.resize((size_t)nb);
      key_of[sd].resize((size_t)nb);
      const int kd = kind[s];
      for (int64_t j = 0; j < nb; ++j) {
        int32_t t = bd[j] + lag * sd;
        if (kd >= 0)
          for (int64_t q = ri.off[kd][j]; q < ri.off[kd][j + 1]; ++q) {
            const int dl = ri.delta[kd][q];
            if (dl <= sd) t = std::max(t, tm[(sd - dl) % 3][ri.block[kd][q]] + gap);
          }
        cur[j] = t;
        t_max = std::max(t_max, t);
        key_of[sd][j] = t * d + sd;
      }
    }
    bucket.assign((size_t)(t_max + 1) * d + 1, 0);
    for (int sd = 0; sd < d; ++sd) for (int32_t k : key_of[sd]) ++bucket[(size_t)k + 1];
    for (size_t k = 0; k + 1 < bucket.size(); ++k) bucket[k + 1] += bucket[k];
    for (int sd = 0; sd < d; ++sd) {
      const int s = s0 + sd;
      const int64_t nb = ri.t[tmpl[s]].nb;
      for (int64_t j = 0; j < nb; ++j) {
        const int64_t t = at + bucket[key_of[sd][j]]++;
        o.new_of[base[s] + j] = (int32_t)t; o.tk_step[t] = s; o.tk_block[t] = (int32_t)j;
      }
    }
    for (int sd = 0; sd < d; ++sd) at += ri.t[tmpl[s0 + sd]].nb;
  }
  o.group_begin.push_back(at);
}

std::string joined_pass_tables(const RotationInfo& ri, const JoinedOrder& ord, int n, bool periodic, JoinedTables& out, FILE* log) {
  const auto t_begin = std::chrono::steady_clock::now();
  auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
  const int depth = ord.depth;
  std::vector<int> tmpl, kind;
  joined_steps(n, tmpl, kind);
  const int n_steps = (int)tmpl.size();
  std::vector<int64_t> nb((size_t)n_steps), base((size_t)n_steps + 1, 0);
  for (int s = 0; s < n_steps; ++s) { nb[s] = ri.t[tmpl[s]].nb; base[s + 1] = base[s] + nb[s]; }
  const int64_t N = base[n_steps];
  if (N > (int64_t)48 << 20) return "too many tickets";                       // too many tickets for one launch: the caller splits the passes
  TicketOrder o;
  // the band order searches its lag from ord.lag on; the tiled order does not depend on it
  const int lag_end = ord.tiles ? ord.lag : std::max(16, 2 * ord.lag);
  int sub = ord.tiles ? ord.sub : 1;                 // (a skewed tiled order that is refused is tried again as the plain tiled order)
  for (int lag = ord.lag; lag <= lag_end; ++lag) {
    if (ord.tiles && sub > 1) skewed_tile_order(ri, n, *ord.tiles, depth, sub, ord.sub_lag, ord.sub_gap, o);
    else if (ord.tiles) tiled_order(ri, n, *ord.tiles, depth, o);
    else band_order(nb, ord.bands, lag, depth, o);
    if (o.group_begin.back() != N) throw std::runtime_error("rotation chain: ticket count");
    if (log) std::fprintf(log, "lpmp:   %d passes, lag %d: order after %.0f ms\n", n, lag, since());
    // every predecessor must come earlier
    bool ok = true;
    for (int s = 1; s < n_steps && ok; ++s) {
      const int kd = kind[s];
      const auto& off = ri.off[kd];
      for (int64_t j = 0; j < nb[s] && ok; ++j)
        for (int64_t q = off[j]; q < off[j + 1]; ++q)
          if (o.new_of[base[s - ri.delta[kd][q]] + ri.block[kd][q]] >= o.new_of[base[s] + j]) {
            if (log) std::fprintf(log, "lpmp:   lag %d: step %d (kind %d) block %lld of %lld needs block %d of step %d (%lld blocks), %d bands\n", lag, s, kd,
                                  (long long)j, (long long)nb[s], ri.block[kd][q], s - ri.delta[kd][q], (long long)nb[s - ri.delta[kd][q]], ord.bands);
            ok = false; break;
          }
    }
    if (log) std::fprintf(log, "lpmp:   checked after %.0f ms (%s)\n", since(), ok ? "valid" : "a dependency points forward");
    if (!ok && ord.tiles && sub > 1) { sub = 1; --lag; continue; }
    if (!ok && ord.tiles) return "internal: the tiled order broke a dependency";   // (valid by construction)
    if (!ok) continue;
    // dependencies in ticket order
    std::vector<int32_t>& dep_off = out.dep_off;
    std::vector<int32_t>& dep = out.dep;
    dep_off.assign((size_t)N + 1, 0);
    for (int s = 1; s < n_steps; ++s) {
      const auto& off = ri.off[kind[s]];
      for (int64_t j = 0; j < nb[s]; ++j) dep_off[o.new_of[base[s] + j] + 1] = (int32_t)(off[j + 1] - off[j]);
    }
    for (int64_t i = 0; i < N; ++i) dep_off[i + 1] += dep_off[i];
    dep.resize((size_t)dep_off[N]);
    for (int s = 1; s < n_steps; ++s) {
      const int kd = kind[s];
      const auto& off = ri.off[kd];
      for (int64_t j = 0; j < nb[s]; ++j) {
        int32_t* dst = dep.data() + dep_off[o.new_of[base[s] + j]];
        for (int64_t q = off[j]; q < off[j + 1]; ++q) *dst++ = o.new_of[base[s - ri.delta[kd][q]] + ri.block[kd][q]];
      }
    }
    if (log) std::fprintf(log, "lpmp:   dependency lists after %.0f ms (%zu)\n", since(), dep.size());
    out.tk_launch.swap(o.tk_step); out.tk_block.swap(o.tk_block);
    out.per_begin = out.per_len = out.ring = 0;
    if (periodic) {
      // the template is [group 0][group 1][group 2 = the period][tail]; what the kernel's map relies on, checked here:
      // groups 1 and 2 are the same tickets in the same order, the period's and the tail's dependencies all lie in the
      // group before the period or later (they move with the copy), the prologue's before the period
      const auto& gb = o.group_begin;
      if (gb.size() != 5) throw std::runtime_error("rotation chain: template groups");
      const int64_t g1 = gb[1], g2 = gb[2], g3 = gb[3], P = g3 - g2;
      const auto& tk_launch = out.tk_launch;
      const auto& tk_block = out.tk_block;
      bool fine = g2 - g1 == P;
      for (int64_t t = g2; t < g3 && fine; ++t) {
        fine = tk_launch[t] == tk_launch[t - P] + depth && tk_block[t] == tk_block[t - P];
        for (int64_t q = dep_off[t]; q < dep_off[t + 1] && fine; ++q) fine = dep[q] >= g1;
      }
      for (int64_t t = g3; t < N && fine; ++t) for (int64_t q = dep_off[t]; q < dep_off[t + 1] && fine; ++q) fine = dep[q] >= g2;
      for (int64_t t = 0; t < g2 && fine; ++t) for (int64_t q = dep_off[t]; q < dep_off[t + 1] && fine; ++q) fine = dep[q] < g2;
      // (group 2's dependencies into group 1 must be what a later copy's are into the copy before it: same relative offsets
      // as group 1's own... group 1 reaches into group 0, whose order differs, so that cannot be compared — the step kinds
      // of groups >= 2 are identical by construction: kind[s] depends on the parity of s only from s = 3 on)
      if (!fine) throw std::runtime_error("rotation chain: the template is not periodic");
      out.per_begin = (int32_t)g2; out.per_len = (int32_t)P;
      // flags: a ring of three groups — a dependency reaches at most into the group before, and a ticket may only publish
      // into a slot whose previous occupant (a ring earlier) has published (kernels.hip, chain_wait)
      out.ring = (int32_t)(3 * P);
    }
    // per-pass bound rows (only written when the launch is given rows: speculative batches): W of pass i (step 2 i + 1)
    // and K after pass i (step 2 i + 2) write row i, for the passes i = 0 ... n - 2 that have a seam behind them
    // (periodic template: every W carries its row — whether it has a seam behind it depends on the call, and the kernel drops
    // rows >= ChainArgs::hist_rows, kernels.hpp)
    out.step_tmpl = tmpl;
    out.step_row.assign((size_t)n_steps, -1);
    for (int s = 0; s < n_steps; ++s) {
      if (tmpl[s] == 1 && ((s - 1) / 2 < n - 1 || periodic)) out.step_row[s] = (s - 1) / 2;
      if (tmpl[s] == 2) out.step_row[s] = (s - 2) / 2;
    }
    out.lag = lag; out.sub = sub;
    return "";
  }
  return "no band order keeps the dependencies backwards";
}

std::vector<int32_t> ticket_descriptors(const std::vector<int32_t>& tk_launch, const std::vector<int32_t>& tk_block, const std::vector<int32_t>& dep_off,
                                        const std::vector<int32_t>& dep, int cap) {
  const size_t N = tk_launch.size();
  if (tk_block.size() != N || dep_off.size() != N + 1 || (N > 0 && (size_t)dep_off[N] != dep.size())) throw std::runtime_error("ticket descriptors: inconsistent ticket tables");
  cap = std::min(std::max(cap, 0), TICKET_DESC_INLINE);
  std::vector<int32_t> d(N * TICKET_DESC_WORDS, -1);
  for (size_t t = 0; t < N; ++t) {
    int32_t* w = d.data() + t * TICKET_DESC_WORDS;
    const int32_t n = dep_off[t + 1] - dep_off[t], ni = std::min<int32_t>(n, cap);
    w[TD_LAUNCH] = tk_launch[t]; w[TD_BLOCK] = tk_block[t]; w[TD_NDEPS] = n; w[TD_REST] = dep_off[t] + ni;
    for (int32_t i = 0; i < ni; ++i) w[TD_DEPS + i] = dep[(size_t)dep_off[t] + i];
  }
  return d;
}

std::vector<int64_t> ticket_dep_histogram(const std::vector<int32_t>& dep_off, int max_count) {
  std::vector<int64_t> h((size_t)std::max(max_count, 0) + 1, 0);
  for (size_t t = 0; t + 1 < dep_off.size(); ++t) ++h[(size_t)std::min<int32_t>(dep_off[t + 1] - dep_off[t], (int32_t)h.size() - 1)];
  return h;
}

}  // namespace lpmp
