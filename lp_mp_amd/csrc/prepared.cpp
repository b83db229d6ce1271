// prepared.cpp — the prepared sets of the C ABI (include/lpmp_engine.h): read-outs, window sets, path sets and forest sets.
// Each is made once for the uploaded model — the planner's checks (plan.cpp), then the device records with the offsets of that
// model, uploaded at create — and a call on it plans and uploads nothing but its inputs.  Host code only, like engine.cpp, whose
// model and entry steps it uses through engine_state.hpp.
#include <functional>
#include <limits>

#include "engine_state.hpp"

// ---- what the four kinds share -----------------------------------------------------------------------------------------------------
// A set remembers the device and the model it was made for (ModelState::model_gen: unique over all engines of the process)
struct PreparedSet { int device = 0; uint64_t gen = 0; };

// entry of a create: there is a model to list factors of; a new set is stamped with it
static void enter_create(lpmp_engine* e, const std::string& who, const char* what) {
  if (!e || !e->model.plan) throw StateError(who + ": no model uploaded (a " + what + " lists factors of the uploaded model)");
}
template <class Set>
static std::unique_ptr<Set> new_set(lpmp_engine* e) {
  auto s = std::make_unique<Set>();
  s->device = e->device; s->gen = e->model.model_gen;
  return s;
}
template <class Set>
static void destroy_set(Set* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  delete s;
}
// entry of a call on a set: the set belongs to the uploaded model (`what` it is and the call it was `made_by` word the refusal),
// validate() judges the call's own arguments on the host, then the engine's device is current and passes that ran ahead are
// settled: the state the call reads or writes is that of the pass the caller is at
template <class Validate>
static void enter_set(lpmp_engine* e, const PreparedSet* set, const std::string& who, const char* what, const char* made_by, Validate&& validate) {
  if (!e || !set) throw std::runtime_error(who + ": null argument");
  if (!e->model.plan || set->gen != e->model.model_gen)
    throw StateError(who + ": the " + what + " was made for another model (lpmp_upload_model since " + made_by + ")");
  validate();
  HIP_CHECK(hipSetDevice(e->device));
  settle(e);
}
// a planner's answer, or its refusal as LPMP_ERR_UNSUPPORTED (PathPlan / ForestPlan / WindowPlan::why)
template <class P>
static P or_refuse(P plan) {
  if (!plan.why.empty()) throw UnsupportedError(plan.why);
  return plan;
}
// a record table of a set: exactly what fill_device does, and nothing at all for an empty one
template <class T>
static void upload_records(DevBuf<T>& dst, const std::vector<T>& src, hipStream_t stream) {
  if (!src.empty()) fill_device(dst, src, stream);
}
// a node's slot in the back-pointer scratch of its group: `count` entries of one byte each, or of two (wide) from an even byte.
// Returns where the slot starts and moves `bytes` past it
static int64_t back_slot(int64_t& bytes, int32_t wide, int64_t count) {
  bytes = (bytes + wide) & ~(int64_t)wide;
  const int64_t off = bytes;
  bytes += count * (wide ? 2 : 1);
  return off;
}
// lpmp_path_moves / lpmp_forest_moves around their launches: the labels every listed unary is relabelled against are those of the
// primal array (ensure_label_array: on a model the rounding code does not take, the array of unset labels — the listed unaries get
// labels, no pairwise slot is written); launch_round issues one round of the set's n_launches launches
template <class LaunchRound>
static int run_moves(lpmp_engine* e, const PreparedSet* set, const std::string& who, const char* what, const char* made_by, size_t n_launches,
                     int rounds, LaunchRound&& launch_round) {
  return guarded([&] {
    enter_set(e, set, who, what, made_by, [&] { if (rounds < 0) throw std::runtime_error(who + ": negative number of rounds"); });
    require_consts(e);
    ensure_label_array(e);
    if (rounds == 0 || n_launches == 0) return;
    ModelState& m = e->model;
    rows_refresh(e);           // (reads the rows; writes no dual)
    for (int r = 0; r < rounds; ++r) launch_round(m);
    if (m.have_primal) launch_primal_propagate(m.d_plinks, m.n_plinks, m.d_primal, e->stream);   // every message's pairwise slot := its unary's label
    HIP_CHECK(hipGetLastError());
  });
}

// ---- path moves: exact relabelling of whole paths given all other labels (include/lpmp_engine.h) ----------------------
// The planner's checks and path edges (plan.cpp, path_plan), then the device records with the offsets of the uploaded model (rows
// layout, float tables and SHARED / DIFF cells are all behind Plan::doff / coff, as in ensure_decode) and the back-pointer scratch
struct lpmp_path_set : PreparedSet {
  int64_t n_groups = 0, n_paths = 0, longest = 0, scratch_bytes = 0;
  DevBuf<PathRec> paths; DevBuf<PathNode> nodes; DevBuf<PathLink> links;
  DevBuf<unsigned char> back;           // back-pointers of one group at a time (launches on one stream follow each other)
  struct Launch { int64_t first, count; int32_t wide, group; };   // per group: its paths of the wave form, then those of the workgroup form
  std::vector<Launch> launches;
};

int lpmp_plan_path_info(lpmp_plan* p, int64_t n_groups, const int64_t* group_off, const int64_t* path_off, const int32_t* unaries,
                        int64_t* n_paths, int64_t* n_path_edges, int64_t* n_off_path_links, char* why, int why_n) {
  if (why && why_n > 0) why[0] = 0;
  const int rc = guarded([&] {
    if (!p) throw std::runtime_error("lpmp_plan_path_info: bad argument");
    const PathPlan pp = or_refuse(p->p.path_plan(n_groups, group_off, path_off, unaries, "lpmp_plan_path_info"));
    if (n_paths) *n_paths = (int64_t)pp.path_off.size() - 1;
    if (n_path_edges) *n_path_edges = pp.n_path_edges;
    if (n_off_path_links) *n_off_path_links = pp.n_off_path_links;
  });
  copy_why(rc, why, why_n);
  return rc;
}

int lpmp_path_set_create(lpmp_engine* e, int64_t n_groups, const int64_t* group_off, const int64_t* path_off, const int32_t* unaries, lpmp_path_set** out) {
  return guarded([&] {
    enter_create(e, "lpmp_path_set_create", "path set");
    if (!out) throw std::runtime_error("lpmp_path_set_create: bad argument");
    HIP_CHECK(hipSetDevice(e->device));
    ModelState& m = e->model;
    const Plan& p = m.plan->p;
    const PathPlan pp = or_refuse(p.path_plan(n_groups, group_off, path_off, unaries, "lpmp_path_set_create"));
    auto ps = new_set<lpmp_path_set>(e);
    ps->n_groups = n_groups; ps->n_paths = (int64_t)pp.path_off.size() - 1; ps->longest = pp.longest;
    const size_t ne = pp.unaries.size();
    std::vector<PathRec> paths; paths.reserve((size_t)ps->n_paths);
    std::vector<PathNode> nodes(ne);
    std::vector<PathLink> links(pp.links.size());
    for (size_t k = 0; k < links.size(); ++k) {
      const PathLinkPlan& l = pp.links[k];
      links[k] = {p.doff(l.p) + (l.side ? p.f_dim0[l.p] : 0), p.coff(l.p), p.f_kind[l.p], p.f_dim1[l.p], l.side, l.other, p.f_dim0[l.other], l.on_path};
    }
    for (int64_t g = 0; g < n_groups; ++g) {
      int64_t bytes = 0;                // of this group's back-pointers: d0 entries per node behind the first of its path
      std::vector<int64_t> form[2];     // the group's paths by form
      for (int64_t j = pp.group_off[(size_t)g]; j < pp.group_off[(size_t)g + 1]; ++j) {
        int32_t widest = 0;
        for (int64_t en = pp.path_off[(size_t)j]; en < pp.path_off[(size_t)j + 1]; ++en) {
          const int32_t u = pp.unaries[(size_t)en], d = p.f_dim0[u], pw = pp.edge[(size_t)en];
          if (d < 1) throw std::runtime_error("lpmp_path_set_create: factor " + std::to_string(u) + " (entry " + std::to_string(en) + ") has no label");
          widest = std::max(widest, d);
          PathNode nd{p.doff(u), 0, 0, d, u, (int32_t)pp.link_off[(size_t)en], (int32_t)(pp.link_off[(size_t)en + 1] - pp.link_off[(size_t)en]), -1, 0, 0, 0};
          if (pw >= 0) {
            const int32_t dprev = p.f_dim0[pp.unaries[(size_t)en - 1]];
            nd.edge_const = p.coff(pw); nd.edge_kind = p.f_kind[pw]; nd.edge_d1 = p.f_dim1[pw]; nd.edge_prev_side = pp.edge_prev_side[(size_t)en];
            nd.back_wide = dprev > 256 ? 1 : 0;
            nd.back_off = back_slot(bytes, nd.back_wide, d);
          }
          nodes[(size_t)en] = nd;
        }
        form[widest > PATH_WAVE_MAX ? 1 : 0].push_back(j);
      }
      ps->scratch_bytes = std::max(ps->scratch_bytes, bytes);
      for (int w = 0; w < 2; ++w) {
        if (form[w].empty()) continue;
        ps->launches.push_back({(int64_t)paths.size(), (int64_t)form[w].size(), w, (int32_t)g});
        for (int64_t j : form[w]) paths.push_back({pp.path_off[(size_t)j], (int32_t)(pp.path_off[(size_t)j + 1] - pp.path_off[(size_t)j]), 0});
      }
    }
    upload_records(ps->paths, paths, e->stream);
    upload_records(ps->nodes, nodes, e->stream);
    upload_records(ps->links, links, e->stream);
    if (ps->scratch_bytes > 0) ps->back.alloc((size_t)ps->scratch_bytes);
    ++m.schedules_built;   // the record tables: structure, like a schedule, counted once
    *out = ps.release();
  });
}
void lpmp_path_set_destroy(lpmp_path_set* ps) { destroy_set(ps); }
int64_t lpmp_path_set_n_groups(const lpmp_path_set* ps) { return ps ? ps->n_groups : 0; }
int64_t lpmp_path_set_n_paths(const lpmp_path_set* ps) { return ps ? ps->n_paths : 0; }
int64_t lpmp_path_set_longest(const lpmp_path_set* ps) { return ps ? ps->longest : 0; }
int64_t lpmp_path_set_scratch_bytes(const lpmp_path_set* ps) { return ps ? ps->scratch_bytes : 0; }

int lpmp_path_moves(lpmp_engine* e, lpmp_path_set* ps, int rounds) {
  return run_moves(e, ps, "lpmp_path_moves", "path set", "lpmp_path_set_create", ps ? ps->launches.size() : 0, rounds, [&](ModelState& m) {
    for (const auto& l : ps->launches)
      launch_path_moves(ps->paths, ps->nodes, ps->links, m.d_dual, m.d_const, m.d_primal, ps->back, l.first, l.count, l.wide, m.tab_flag, e->stream);
  });
}

// ---- forest moves: exact relabelling of induced forests given all other labels (include/lpmp_engine.h) -----------------
// The path set's twin for trees: the planner's checks, tree edges, children, heights and depths (plan.cpp, forest_plan), then the
// device records, the launch lists (per group: the nodes by height and form for the up sweep, by depth for the down sweep) and the
// scratch of rows and back-pointers of the largest group
struct lpmp_forest_set : PreparedSet {
  int64_t n_groups = 0, n_trees = 0, max_height = 0, scratch_bytes = 0;
  DevBuf<ForestNode> nodes; DevBuf<PathLink> links; DevBuf<int64_t> child_g; DevBuf<int32_t> list;
  DevBuf<double> rows; DevBuf<unsigned char> back;      // of one group at a time (launches on one stream follow each other)
  struct Launch { int64_t first, count; int32_t wide; };            // wide < 0: a level of the down sweep
  std::vector<Launch> launches;
};

int lpmp_plan_forest_info(lpmp_plan* p, int64_t n_groups, const int64_t* group_off, const int32_t* unaries, const int32_t* parent,
                          int64_t* n_trees, int64_t* n_tree_edges, int64_t* n_off_tree_links, int64_t* max_height, char* why, int why_n) {
  if (why && why_n > 0) why[0] = 0;
  const int rc = guarded([&] {
    if (!p) throw std::runtime_error("lpmp_plan_forest_info: bad argument");
    const ForestPlan fp = or_refuse(p->p.forest_plan(n_groups, group_off, unaries, parent, "lpmp_plan_forest_info"));
    if (n_trees) *n_trees = fp.n_trees;
    if (n_tree_edges) *n_tree_edges = fp.n_tree_edges;
    if (n_off_tree_links) *n_off_tree_links = fp.n_off_tree_links;
    if (max_height) *max_height = fp.max_height;
  });
  copy_why(rc, why, why_n);
  return rc;
}

int lpmp_plan_suggest_forests(lpmp_plan* p, int64_t max_groups, int64_t* n_groups, int64_t* n_entries, int64_t* group_off, int32_t* unaries,
                              int32_t* parent, int64_t* n_left_out) {
  return guarded([&] {
    if (!p || max_groups < 0) throw std::runtime_error("lpmp_plan_suggest_forests: bad argument");
    const ForestCover fc = suggest_forests(p->p, max_groups);
    if (n_groups) *n_groups = (int64_t)fc.group_off.size() - 1;
    if (n_entries) *n_entries = (int64_t)fc.unaries.size();
    if (n_left_out) *n_left_out = fc.n_left_out;
    if (group_off) std::copy(fc.group_off.begin(), fc.group_off.end(), group_off);
    if (unaries) std::copy(fc.unaries.begin(), fc.unaries.end(), unaries);
    if (parent) std::copy(fc.parent.begin(), fc.parent.end(), parent);
  });
}

int lpmp_forest_set_create(lpmp_engine* e, int64_t n_groups, const int64_t* group_off, const int32_t* unaries, const int32_t* parent, lpmp_forest_set** out) {
  return guarded([&] {
    enter_create(e, "lpmp_forest_set_create", "forest set");
    if (!out) throw std::runtime_error("lpmp_forest_set_create: bad argument");
    HIP_CHECK(hipSetDevice(e->device));
    ModelState& m = e->model;
    const Plan& p = m.plan->p;
    const ForestPlan fp = or_refuse(p.forest_plan(n_groups, group_off, unaries, parent, "lpmp_forest_set_create"));
    auto fs = new_set<lpmp_forest_set>(e);
    fs->n_groups = n_groups; fs->n_trees = fp.n_trees; fs->max_height = fp.max_height;
    const size_t ne = fp.unaries.size();
    std::vector<ForestNode> nodes(ne);
    std::vector<PathLink> links(fp.links.size());
    std::vector<int64_t> child_g(fp.children.size());
    std::vector<int32_t> list; list.reserve(2 * ne);
    for (size_t k = 0; k < links.size(); ++k) {
      const ForestLinkPlan& l = fp.links[k];
      links[k] = {p.doff(l.p) + (l.side ? p.f_dim0[l.p] : 0), p.coff(l.p), p.f_kind[l.p], p.f_dim1[l.p], l.side, l.other, p.f_dim0[l.other], l.tree ? 1 : 0};
    }
    int64_t max_rows = 0, max_back = 0;
    std::vector<std::vector<int32_t>> up[2], down;     // the group's entries by height and form, and by depth
    for (int64_t g = 0; g < n_groups; ++g) {
      const int64_t gb = fp.group_off[(size_t)g], ge = fp.group_off[(size_t)g + 1];
      if (gb == ge) continue;
      const size_t levels = (size_t)fp.group_height[(size_t)g] + 1;
      for (int w = 0; w < 2; ++w) up[w].assign(levels, {});
      down.assign(levels, {});
      int64_t n_rows = 0, bytes = 0;    // of this group's rows (doubles) and back-pointers
      for (int64_t en = gb; en < ge; ++en) {
        const int32_t u = fp.unaries[(size_t)en], d = p.f_dim0[u], q = fp.parent_entry[(size_t)en], pw = fp.edge[(size_t)en];
        if (d < 1) throw std::runtime_error("lpmp_forest_set_create: factor " + std::to_string(u) + " (entry " + std::to_string(en) + ") has no label");
        ForestNode nd{p.doff(u), 0, 0, 0, d, u, (int32_t)fp.link_off[(size_t)en], (int32_t)(fp.link_off[(size_t)en + 1] - fp.link_off[(size_t)en]), -1, 0, 0, 0, 0, -1,
                      (int32_t)fp.child_off[(size_t)en], (int32_t)(fp.child_off[(size_t)en + 1] - fp.child_off[(size_t)en])};
        int32_t widest = d;
        if (q >= 0) {
          const int32_t dq = p.f_dim0[fp.unaries[(size_t)q]];
          widest = std::max(widest, dq);
          nd.edge_const = p.coff(pw); nd.edge_kind = p.f_kind[pw]; nd.edge_d1 = p.f_dim1[pw]; nd.edge_side = fp.edge_side[(size_t)en];
          nd.dq = dq; nd.parent = fp.unaries[(size_t)q];
          nd.g_off = n_rows; n_rows += dq;
          nd.back_wide = d > 256 ? 1 : 0;
          nd.back_off = back_slot(bytes, nd.back_wide, dq);
          down[(size_t)fp.depth[(size_t)en]].push_back((int32_t)en);
        }
        nodes[(size_t)en] = nd;
        up[widest > PATH_WAVE_MAX ? 1 : 0][(size_t)fp.height[(size_t)en]].push_back((int32_t)en);
      }
      max_rows = std::max(max_rows, n_rows); max_back = std::max(max_back, bytes);
      for (size_t h = 0; h < levels; ++h)
        for (int w = 0; w < 2; ++w) {
          if (up[w][h].empty()) continue;
          fs->launches.push_back({(int64_t)list.size(), (int64_t)up[w][h].size(), w});
          list.insert(list.end(), up[w][h].begin(), up[w][h].end());
        }
      for (size_t dp = 1; dp < levels; ++dp) {
        if (down[dp].empty()) continue;
        fs->launches.push_back({(int64_t)list.size(), (int64_t)down[dp].size(), -1});
        list.insert(list.end(), down[dp].begin(), down[dp].end());
      }
    }
    for (size_t k = 0; k < child_g.size(); ++k) child_g[k] = nodes[(size_t)fp.children[k]].g_off;
    fs->scratch_bytes = 8 * max_rows + max_back;
    upload_records(fs->nodes, nodes, e->stream);
    upload_records(fs->links, links, e->stream);
    upload_records(fs->child_g, child_g, e->stream);
    upload_records(fs->list, list, e->stream);
    if (max_rows > 0) fs->rows.alloc((size_t)max_rows);
    if (max_back > 0) fs->back.alloc((size_t)max_back);
    ++m.schedules_built;   // the record tables: structure, like a schedule, counted once
    *out = fs.release();
  });
}
void lpmp_forest_set_destroy(lpmp_forest_set* fs) { destroy_set(fs); }
int64_t lpmp_forest_set_n_groups(const lpmp_forest_set* fs) { return fs ? fs->n_groups : 0; }
int64_t lpmp_forest_set_n_trees(const lpmp_forest_set* fs) { return fs ? fs->n_trees : 0; }
int64_t lpmp_forest_set_max_height(const lpmp_forest_set* fs) { return fs ? fs->max_height : 0; }
int64_t lpmp_forest_set_scratch_bytes(const lpmp_forest_set* fs) { return fs ? fs->scratch_bytes : 0; }

int lpmp_forest_moves(lpmp_engine* e, lpmp_forest_set* fs, int rounds) {
  return run_moves(e, fs, "lpmp_forest_moves", "forest set", "lpmp_forest_set_create", fs ? fs->launches.size() : 0, rounds, [&](ModelState& m) {
    for (const auto& l : fs->launches) {
      if (l.wide < 0) launch_forest_down(fs->list, fs->nodes, m.d_primal, fs->back, l.first, l.count, e->stream);
      else launch_forest_up(fs->list, fs->nodes, fs->child_g, fs->links, m.d_dual, m.d_const, m.d_primal, fs->rows, fs->back, l.first, l.count, l.wide, m.tab_flag, e->stream);
    }
  });
}

// ---- prepared read-outs: labels, unaries and beliefs of listed VECTOR factors into the caller's array (include/lpmp_engine.h) -------
// The output twin of lpmp_set_vectors, prepared like a schedule: the record list is uploaded at create, a call uploads nothing.
struct lpmp_readout : PreparedSet {
  int64_t n = 0;
  int32_t max_labels = 0;
  std::vector<int32_t> factors, d0;     // the list, and every row's label count (a host destination is filled row by row)
  DevBuf<ReadoutRec> recs;              // in the caller's order: row i = record i
  int32_t unsupported = -1;             // lowest listed factor with a message the beliefs do not take (-1: none)
  std::string why;
  int32_t duplicate = -1;               // lowest factor listed twice (-1: none): lpmp_readout_set_labels refuses the read-out
  // beliefs: the records again, sorted by label-count class, with their links in message-list order; built on the first call
  struct Launch { int64_t first, count; int32_t width; };
  bool have_links = false;
  DevBuf<ReadoutRec> brecs; DevBuf<DecodeLink> links;
  std::vector<Launch> launches;
};

static int readout_class(int32_t d0) { return d0 <= 4 ? 0 : d0 <= 8 ? 1 : d0 <= 16 ? 2 : d0 <= READOUT_GROUP_MAX ? 3 : d0 <= 64 ? 4 : 5; }
static const int32_t READOUT_CLASS_WIDTH[6] = {4, 8, 16, READOUT_GROUP_MAX, 64, GEN_MAXD};

// the link tables of the beliefs: a function of the structure, like a schedule, and counted as one
static void ensure_readout_links(lpmp_engine* e, lpmp_readout* r) {
  if (r->have_links) return;
  r->brecs.reset(); r->links.reset(); r->launches.clear();
  const Plan& p = e->model.plan->p;
  int64_t start[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int64_t i = 0; i < r->n; ++i) ++start[readout_class(r->d0[(size_t)i]) + 1];
  for (int c = 0; c < 6; ++c) start[c + 1] += start[c];
  std::vector<ReadoutRec> recs((size_t)r->n);
  std::vector<DecodeLink> links;
  std::vector<int64_t> begin_of((size_t)p.nf, -1);   // a factor listed twice shares its links
  int64_t cur[6];
  for (int c = 0; c < 6; ++c) cur[c] = start[c];
  for (int64_t i = 0; i < r->n; ++i) {
    const int32_t u = r->factors[(size_t)i];
    const int64_t a = p.fm_off[(size_t)u], b = p.fm_off[(size_t)u + 1];
    if (begin_of[(size_t)u] < 0) {
      begin_of[(size_t)u] = (int64_t)links.size();
      for (int64_t k = a; k < b; ++k) {   // the order of the message list: the order in which a sweep receives
        const int32_t msg = p.fm[(size_t)k].msg, pw = p.m_right[(size_t)msg];
        links.push_back({p.doff(pw), p.coff(pw), p.f_kind[pw], p.f_dim0[pw], p.f_dim1[pw], p.mtypes[(size_t)p.m_type[(size_t)msg]].param, 0, 0});
      }
      if (links.size() > (size_t)std::numeric_limits<int32_t>::max()) throw std::runtime_error("lpmp_readout_beliefs: more than 2^31 links");
    }
    recs[(size_t)cur[readout_class(r->d0[(size_t)i])]++] = {p.f_doff[(size_t)u], i, r->d0[(size_t)i], u, (int32_t)begin_of[(size_t)u], (int32_t)(b - a)};
  }
  for (int c = 0; c < 6; ++c) if (start[c + 1] > start[c]) r->launches.push_back({start[c], start[c + 1] - start[c], READOUT_CLASS_WIDTH[c]});
  upload_records(r->brecs, recs, e->stream);
  upload_records(r->links, links, e->stream);
  r->have_links = true;
  ++e->model.schedules_built;
}

int lpmp_readout_create(lpmp_engine* e, int64_t n, const int32_t* factors, lpmp_readout** out) {
  return guarded([&] {
    enter_create(e, "lpmp_readout_create", "read-out");
    if (!out || (factors && n < 0)) throw std::runtime_error("lpmp_readout_create: bad argument");
    HIP_CHECK(hipSetDevice(e->device));
    const Plan& p = e->model.plan->p;
    auto r = new_set<lpmp_readout>(e);
    if (!factors) { for (int64_t f = 0; f < p.nf; ++f) if (p.f_kind[f] == LPMP_F_VECTOR) r->factors.push_back((int32_t)f); }
    else {
      r->factors.reserve((size_t)n);
      for (int64_t i = 0; i < n; ++i) {
        const int32_t f = factors[i];
        if (f < 0 || f >= p.nf) throw std::runtime_error("lpmp_readout_create: factor index " + std::to_string(f) + " (entry " + std::to_string(i) + ") is out of range");
        if (p.f_kind[f] != LPMP_F_VECTOR) throw std::runtime_error("lpmp_readout_create: factor " + std::to_string(f) + " is not a VECTOR factor");
        r->factors.push_back(f);
      }
    }
    r->n = (int64_t)r->factors.size();
    if (factors) {   // (reads are idempotent; a write of two rows into one slot is not: decided here, refused in lpmp_readout_set_labels)
      std::vector<uint8_t> seen((size_t)p.nf, 0);
      for (const int32_t f : r->factors) {
        if (seen[(size_t)f] && (r->duplicate < 0 || f < r->duplicate)) r->duplicate = f;
        seen[(size_t)f] = 1;
      }
    }
    std::vector<ReadoutRec> recs((size_t)r->n);
    r->d0.resize((size_t)r->n);
    for (int64_t i = 0; i < r->n; ++i) {
      const int32_t f = r->factors[(size_t)i], len = p.f_dim0[f];
      r->d0[(size_t)i] = len;
      r->max_labels = std::max(r->max_labels, len);
      recs[(size_t)i] = {p.f_doff[f], i, len, f, 0, 0};
      // beliefs: every message of the factor is a unary-pairwise one with the factor on its left (the unary) and a pairwise factor on its right
      for (int64_t k = p.fm_off[(size_t)f]; k < p.fm_off[(size_t)f + 1]; ++k) {
        const MsgEntry& me = p.fm[(size_t)k];
        const bool ok = p.mtypes[(size_t)p.m_type[(size_t)me.msg]].kind == LPMP_M_UNARY_PAIRWISE && me.role == 0 && p.f_kind[p.m_right[(size_t)me.msg]] != LPMP_F_VECTOR;
        if (!ok && (r->unsupported < 0 || f < r->unsupported)) r->unsupported = f;
      }
    }
    if (r->unsupported >= 0)
      r->why = "lpmp_readout_beliefs: factor " + std::to_string(r->unsupported) + " has a message that is not a unary-pairwise message with the factor as its unary (DESIGN.md 8)";
    upload_records(r->recs, recs, e->stream);
    *out = r.release();
  });
}
void lpmp_readout_destroy(lpmp_readout* r) { destroy_set(r); }
int64_t lpmp_readout_n(const lpmp_readout* r) { return r ? r->n : 0; }
int32_t lpmp_readout_max_labels(const lpmp_readout* r) { return r ? r->max_labels : 0; }

// common entry of the three reading calls: the read-out belongs to the uploaded model, the arguments are usable
static void readout_enter(lpmp_engine* e, lpmp_readout* r, const void* dst, int dst_mem, const int64_t* dst_stride, const std::string& who) {
  enter_set(e, r, who, "read-out", "lpmp_readout_create", [&] {
    if (dst_mem != LPMP_MEM_HOST && dst_mem != LPMP_MEM_DEVICE) throw std::runtime_error(who + ": dst_mem must be LPMP_MEM_HOST or LPMP_MEM_DEVICE");
    if (r->n > 0 && !dst) throw std::runtime_error(who + ": null destination");
    if (dst_stride && *dst_stride < r->max_labels)
      throw std::runtime_error(who + ": dst_stride " + std::to_string(*dst_stride) + " is smaller than the " + std::to_string(r->max_labels) + " entries of the longest listed vector");
  });
  // a DEVICE destination never waits for the stream, as lpmp_decode_primal does not: an aborted chain run is reported by the next
  // call that synchronises anyway.  A HOST destination ends in a synchronising copy and reports it here
  if (dst_mem == LPMP_MEM_HOST) check_chain(e);
}
// rows of doubles: straight into a device destination, or into the engine's buffer (rows max_labels apart) and from there, row by
// row, into the entries of the host destination that belong to a factor
static void readout_rows(lpmp_engine* e, lpmp_readout* r, double* dst, int64_t dst_stride, int dst_mem, const std::function<void(double*, int64_t)>& launch) {
  if (dst_mem == LPMP_MEM_DEVICE) { launch(dst, dst_stride); HIP_CHECK(hipGetLastError()); return; }
  const size_t total = (size_t)r->n * (size_t)r->max_labels;
  if (total == 0) return;
  e->model.d_readout.grow(total);
  launch(e->model.d_readout.get(), (int64_t)r->max_labels);
  HIP_CHECK(hipGetLastError());
  // (whole rows, one staging chunk at a time: no second buffer of the size of the read-out on the host)
  const int64_t L = r->max_labels, per = std::max<int64_t>(1, (int64_t)(STAGE_CHUNK / sizeof(double)) / L);
  std::vector<double> rows((size_t)(std::min(per, r->n) * L));
  for (int64_t first = 0; first < r->n; first += per) {
    const int64_t cnt = std::min(per, r->n - first);
    d2h(rows.data(), e->model.d_readout.get() + first * L, (size_t)(cnt * L) * sizeof(double), e->stream);
    for (int64_t i = 0; i < cnt; ++i)
      std::copy(rows.begin() + i * L, rows.begin() + i * L + r->d0[(size_t)(first + i)], dst + (first + i) * dst_stride);
  }
}

int lpmp_readout_labels(lpmp_engine* e, lpmp_readout* r, int32_t* dst, int dst_mem) {
  return guarded([&] {
    readout_enter(e, r, dst, dst_mem, nullptr, "lpmp_readout_labels");
    if (r->n == 0) return;
    ensure_label_array(e);
    if (dst_mem == LPMP_MEM_DEVICE) { launch_readout_labels(r->recs, r->n, e->model.d_primal, dst, e->stream); HIP_CHECK(hipGetLastError()); return; }
    e->model.d_readout.grow(((size_t)r->n + 1) / 2);
    int32_t* stage = reinterpret_cast<int32_t*>(e->model.d_readout.get());
    launch_readout_labels(r->recs, r->n, e->model.d_primal, stage, e->stream);
    HIP_CHECK(hipGetLastError());
    d2h(dst, stage, (size_t)r->n * sizeof(int32_t), e->stream);
  });
}
// the input twin of lpmp_readout_labels (include/lpmp_engine.h)
int lpmp_readout_set_labels(lpmp_engine* e, lpmp_readout* r, const int32_t* src, int src_mem) {
  return guarded([&] {
    const std::string who = "lpmp_readout_set_labels";
    const bool host = src_mem == LPMP_MEM_HOST;
    enter_set(e, r, who, "read-out", "lpmp_readout_create", [&] {
      if (src_mem != LPMP_MEM_HOST && src_mem != LPMP_MEM_DEVICE) throw std::runtime_error(who + ": src_mem must be LPMP_MEM_HOST or LPMP_MEM_DEVICE");
      if (r->n > 0 && !src) throw std::runtime_error(who + ": null source");
      if (r->duplicate >= 0) throw std::runtime_error(who + ": factor " + std::to_string(r->duplicate) + " is listed twice in the read-out (two rows would write one label)");
      if (host)
        for (int64_t i = 0; i < r->n; ++i)
          if (src[i] < 0 || src[i] > r->d0[(size_t)i])
            throw std::runtime_error(who + ": label " + std::to_string(src[i]) + " (entry " + std::to_string(i) + ", factor " + std::to_string(r->factors[(size_t)i]) + ") is outside [0, " +
                                     std::to_string(r->d0[(size_t)i]) + "] (the dimension means unset); nothing was written");
    });
    // (a device source never waits for the stream, as a read-out into device memory does not; a host source ends in a synchronising copy)
    if (host) check_chain(e);
    if (r->n == 0) return;
    ensure_label_array(e);
    ModelState& m = e->model;
    const int32_t* d_src = src;
    if (host) {
      m.d_readout.grow(((size_t)r->n + 1) / 2);
      int32_t* stage = reinterpret_cast<int32_t*>(m.d_readout.get());
      h2d(stage, src, (size_t)r->n * sizeof(int32_t), e->stream);
      d_src = stage;
    }
    launch_set_labels(r->recs, r->n, d_src, m.d_primal, e->stream);
    if (m.have_primal) launch_primal_propagate(m.d_plinks, m.n_plinks, m.d_primal, e->stream);   // every message's pairwise slot := its unary's label
    HIP_CHECK(hipGetLastError());
  });
}
int lpmp_readout_vectors(lpmp_engine* e, lpmp_readout* r, double* dst, int64_t dst_stride, int dst_mem) {
  return guarded([&] {
    readout_enter(e, r, dst, dst_mem, &dst_stride, "lpmp_readout_vectors");
    if (r->n == 0) return;
    // (vector factors live in the packed array under every layout: nothing of the rows is read)
    readout_rows(e, r, dst, dst_stride, dst_mem, [&](double* d, int64_t stride) {
      launch_readout_vectors(r->recs, r->n, r->max_labels, e->model.d_dual, d, stride, e->stream);
    });
  });
}
int lpmp_readout_beliefs(lpmp_engine* e, lpmp_readout* r, double* dst, int64_t dst_stride, int dst_mem) {
  return guarded([&] {
    readout_enter(e, r, dst, dst_mem, &dst_stride, "lpmp_readout_beliefs");
    if (r->unsupported >= 0) throw UnsupportedError(r->why);
    if (r->n == 0) return;
    require_consts(e);
    ensure_readout_links(e, r);
    rows_refresh(e);           // (reads the rows; writes no dual)
    readout_rows(e, r, dst, dst_stride, dst_mem, [&](double* d, int64_t stride) {
      for (const auto& l : r->launches)
        launch_readout_beliefs(r->brecs, r->links, e->model.d_dual, e->model.d_const, d, stride, l.first, l.count, l.width, e->model.tab_flag, e->stream);
    });
  });
}

// ---- moving label windows: duals and shifts carried along on the device (include/lpmp_engine.h) ---------------------------------
// What a window set is made of is the planner's (plan.cpp, window_plan; lpmp_plan_window_info asks a stand-alone plan)
int lpmp_plan_window_info(lpmp_plan* p, int64_t n, const int32_t* factors, int64_t* n_links, int64_t* n_pairwise, char* why, int why_n) {
  if (why && why_n > 0) why[0] = 0;
  const int rc = guarded([&] {
    if (!p || (factors && n < 0)) throw std::runtime_error("lpmp_plan_window_info: bad argument");
    const WindowPlan w = or_refuse(p->p.window_plan(n, factors, "lpmp_plan_window_info"));
    if (n_links) *n_links = (int64_t)w.links.size();
    if (n_pairwise) *n_pairwise = (int64_t)w.pairs.size();
  });
  copy_why(rc, why, why_n);
  return rc;
}

// A prepared list of unaries whose windows move together: records and links are uploaded at create
struct lpmp_window_set : PreparedSet {
  int64_t n = 0, n_pairwise = 0;
  int32_t max_labels = 0;
  DevBuf<MoveRec> recs; DevBuf<MoveLink> links; DevBuf<MoveShiftRec> pairs;
  DevBuf<int32_t> d_delta;              // a host delta, and host costs, pass through buffers of the set
  DevBuf<double> d_cost[2];
};

int lpmp_window_set_create(lpmp_engine* e, int64_t n, const int32_t* factors, lpmp_window_set** out) {
  return guarded([&] {
    enter_create(e, "lpmp_window_set_create", "window set");
    if (!out || (factors && n < 0)) throw std::runtime_error("lpmp_window_set_create: bad argument");
    HIP_CHECK(hipSetDevice(e->device));
    ModelState& m = e->model;
    const Plan& p = m.plan->p;
    const WindowPlan w = or_refuse(p.window_plan(n, factors, "lpmp_window_set_create"));
    auto ws = new_set<lpmp_window_set>(e);
    ws->n = (int64_t)w.factors.size(); ws->n_pairwise = (int64_t)w.pairs.size(); ws->max_labels = w.max_labels;
    std::vector<MoveRec> recs((size_t)ws->n);
    for (int64_t i = 0; i < ws->n; ++i) {
      const int32_t u = w.factors[(size_t)i];
      // (vector factors live in the packed array under every layout)
      recs[(size_t)i] = {p.f_doff[(size_t)u], p.f_dim0[u], u, (int32_t)w.link_off[(size_t)i], (int32_t)(w.link_off[(size_t)i + 1] - w.link_off[(size_t)i]), (int32_t)i, 0};
    }
    std::vector<MoveLink> links(w.links.size());
    for (size_t k = 0; k < links.size(); ++k) links[k] = {p.doff(w.links[k].p) + (w.links[k].side ? p.f_dim0[w.links[k].p] : 0)};
    // the places of a shift: those lpmp_set_constants writes for the second entry of a DIFF_SHIFT row
    const int64_t sh_base = m.d_shared ? (int64_t)(((intptr_t)m.d_shared.get() - (intptr_t)m.d_const) / 8) : 0;
    std::vector<MoveShiftRec> pairs(w.pairs.size());
    for (size_t k = 0; k < pairs.size(); ++k) {
      const int32_t f = w.pairs[k].p;
      const int64_t cell = p.coff(f), c = (cell - sh_base) / 2;
      if (c < 0 || 2 * c + 3 >= (int64_t)m.sh_cells.size() || sh_base + 2 * c != cell) throw std::runtime_error("lpmp_window_set_create: internal: factor " + std::to_string(f) + " has no cell");
      pairs[k] = {cell + 2, m.sh_cells[(size_t)(2 * c + 2)], w.pairs[k].left_row, w.pairs[k].right_row, f, 0};
    }
    upload_records(ws->recs, recs, e->stream);
    upload_records(ws->links, links, e->stream);
    upload_records(ws->pairs, pairs, e->stream);
    ++m.schedules_built;   // the link tables: structure, like a schedule, counted once
    *out = ws.release();
  });
}
void lpmp_window_set_destroy(lpmp_window_set* ws) { destroy_set(ws); }
int64_t lpmp_window_set_n(const lpmp_window_set* ws) { return ws ? ws->n : 0; }
int32_t lpmp_window_set_max_labels(const lpmp_window_set* ws) { return ws ? ws->max_labels : 0; }
int64_t lpmp_window_set_n_pairwise(const lpmp_window_set* ws) { return ws ? ws->n_pairwise : 0; }

// lpmp_move_windows and lpmp_move_windows_carry: one path up to what becomes of the labels
static int move_windows(lpmp_engine* e, lpmp_window_set* ws, const int32_t* delta, int delta_mem, const double* cost_old, const double* cost_new,
                        int64_t cost_stride, int cost_mem, bool carry) {
  return guarded([&] {
    const std::string who = carry ? "lpmp_move_windows_carry" : "lpmp_move_windows";
    const bool costs = cost_old || cost_new;
    const bool host_delta = delta_mem == LPMP_MEM_HOST, host_costs = costs && cost_mem == LPMP_MEM_HOST;
    enter_set(e, ws, who, "window set", "lpmp_window_set_create", [&] {
      require_consts(e);
      if (delta_mem != LPMP_MEM_HOST && delta_mem != LPMP_MEM_DEVICE) throw std::runtime_error(who + ": delta_mem must be LPMP_MEM_HOST or LPMP_MEM_DEVICE");
      if (costs && cost_mem != LPMP_MEM_HOST && cost_mem != LPMP_MEM_DEVICE) throw std::runtime_error(who + ": cost_mem must be LPMP_MEM_HOST or LPMP_MEM_DEVICE");
      if (!cost_old != !cost_new) throw std::runtime_error(who + ": cost_old and cost_new come together (the unary costs in the old and in the new window), or not at all");
      if (ws->n > 0 && !delta) throw std::runtime_error(who + ": null delta");
      if (costs && cost_stride < ws->max_labels)
        throw std::runtime_error(who + ": cost_stride " + std::to_string(cost_stride) + " is smaller than the " + std::to_string(ws->max_labels) + " entries of the longest listed vector");
      if (host_delta)
        for (int64_t i = 0; i < ws->n; ++i)
          if (delta[i] < -MOVE_DELTA_MAX || delta[i] > MOVE_DELTA_MAX)
            throw std::runtime_error(who + ": delta " + std::to_string(delta[i]) + " (entry " + std::to_string(i) + ") is beyond +-2^20; nothing was written");
    });
    // (device inputs never wait for the stream, as a read-out into device memory does not; host inputs end in a synchronisation)
    if (host_delta || host_costs) check_chain(e);
    if (ws->n == 0) return;
    ModelState& m = e->model;
    const int32_t* d_delta = delta;
    if (host_delta) { ws->d_delta.grow((size_t)ws->n); h2d(ws->d_delta, delta, (size_t)ws->n * sizeof(int32_t), e->stream); d_delta = ws->d_delta.get(); }
    const double* d_cost[2] = {cost_old, cost_new};
    if (host_costs) {
      const size_t total = (size_t)(ws->n - 1) * (size_t)cost_stride + (size_t)ws->max_labels;   // (the last row need not be a whole stride)
      for (int k = 0; k < 2; ++k) { ws->d_cost[k].grow(total); h2d(ws->d_cost[k], d_cost[k], total * sizeof(double), e->stream); d_cost[k] = ws->d_cost[k].get(); }
    }
    // (the message vectors of DIFF_SHIFT factors and all vector factors live in the packed array under every layout, and both
    // kernels are plain launches on the engine's stream: never part of a captured graph or a persistent launch)
    launch_move_shifts(ws->pairs, ws->n_pairwise, d_delta, m.d_const, m.d_lb, e->stream);
    launch_move_windows(ws->recs, ws->links, ws->n, d_delta, m.d_dual, m.d_lb, d_cost[0], d_cost[1], cost_stride, e->stream);
    HIP_CHECK(hipGetLastError());
    if (carry) {
      // the labelling is the one piece of state whose meaning is exactly an absolute label: x names x - delta in the new window.  No
      // primal array: none is made.  The pairwise slots follow their unaries as after a decode (primal_unset_only: unaries only)
      if (m.have_primal || m.primal_unset_only) launch_carry_labels(ws->recs, ws->n, d_delta, m.d_primal, e->stream);
      if (m.have_primal) launch_primal_propagate(m.d_plinks, m.n_plinks, m.d_primal, e->stream);
      HIP_CHECK(hipGetLastError());
    } else if (m.have_primal || m.primal_unset_only) { upload_unset_primal(e); m.primal_t = 0; }   // as after lpmp_set_constants: the labels belong to the old windows
    if (host_delta || host_costs) HIP_CHECK(hipStreamSynchronize(e->stream));   // the caller's arrays are the caller's again
  });
}
int lpmp_move_windows(lpmp_engine* e, lpmp_window_set* ws, const int32_t* delta, int delta_mem, const double* cost_old, const double* cost_new,
                      int64_t cost_stride, int cost_mem) {
  return move_windows(e, ws, delta, delta_mem, cost_old, cost_new, cost_stride, cost_mem, false);
}
int lpmp_move_windows_carry(lpmp_engine* e, lpmp_window_set* ws, const int32_t* delta, int delta_mem, const double* cost_old, const double* cost_new,
                            int64_t cost_stride, int cost_mem) {
  return move_windows(e, ws, delta, delta_mem, cost_old, cost_new, cost_stride, cost_mem, true);
}
