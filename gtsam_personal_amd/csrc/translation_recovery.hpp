// TranslationRecovery on the device (gtsam/sfm/TranslationRecovery.cpp:49-228, TranslationFactor.h): host side of the
// lmgpu_translation_recovery_* group.  Included by lmgpu.hip after the handle's own entry points.  A session owns one inner lmgpu_handle
// whose variables are all LMGPU_POINT3 and whose factors are buckets of the internal rows kTranslationType / kBetweenPoint3Type
// (factor_types.hpp) plus one or two public LMGPU_F_PRIOR_POINT3; the solve is lmgpu_optimize on that handle.
#pragma once

#include <random>
#include <set>

struct lmgpu_translation_recovery {
  lmgpu_config cfg{};
  std::string err;
  struct Edge {
    int32_t index;  // position in the caller's list
    uint64_t k1, k2;
    double z[3];
    int32_t noise_kind;
    double noise[9];
    int32_t robust;
    double rk;
  };
  std::vector<Edge> dirs, betw;  // as added
  double prior_sigma = 0.01;     // addPrior's default priorNoiseModel: Isotropic(3, 0.01)
  std::mt19937 rng{42};          // the reference's kRandomNumberGenerator(42) is process-wide; this one belongs to the session
  bool finalized = false;
  // after finalize
  std::vector<uint64_t> keys;       // every key of the input, by first appearance (directions, then betweens)
  std::vector<uint64_t> rep;        // its representative (itself unless merged away by a zero-direction edge)
  std::vector<uint64_t> slot_keys;  // the inner handle's variables = the representatives in elimination order
  std::vector<double> initial;      // [slots][3]
  std::vector<double> result;       // [keys][3]
  bool have_result = false;
  int n_fac = 0, n_dir = 0;
  lmgpu_handle* h = nullptr;  // null when the graph is empty (no direction edge remains: addPrior adds nothing either, :125-126)
};

namespace {

void tr_release(lmgpu_translation_recovery* tr) {
  if (tr->h) lmgpu_destroy(tr->h);
  tr->h = nullptr;
  tr->finalized = false;
  tr->have_result = false;
}

int tr_inner(lmgpu_translation_recovery* tr, int rc) {
  if (rc != LMGPU_OK) tr->err = std::string("inner handle: ") + lmgpu_last_error(tr->h);
  return rc;
}

// one coordinate of initializeRandomly's Point3 (:149,159): uniform in [-1, 1) from two consecutive 32-bit draws, written out because
// std::uniform_real_distribution's algorithm is implementation-defined
double tr_uniform(std::mt19937& g) {
  const double x1 = (double)(uint32_t)g();
  const double x2 = (double)(uint32_t)g();
  return 2.0 * ((x1 + x2 * 4294967296.0) / 18446744073709551616.0) - 1.0;
}

int tr_add(lmgpu_translation_recovery* tr, std::vector<lmgpu_translation_recovery::Edge>& to, const char* who, int32_t n, const int32_t* index,
           const uint64_t* keys, const double* meas, int32_t noise_kind, const double* noise, int32_t robust_kind, double robust_k) {
  if (n < 0 || (noise_kind != LMGPU_N_UNIT && noise_kind != LMGPU_N_DIAG && noise_kind != LMGPU_N_GAUSS) || robust_kind < LMGPU_ROBUST_NONE ||
      robust_kind > LMGPU_ROBUST_L2_WITH_DEAD_ZONE || (robust_kind != LMGPU_ROBUST_NONE && !(robust_k > 0.0))) {
    tr->err = std::string(who) + ": bad count, noise kind or robust kind";
    return LMGPU_INVALID;
  }
  if (n == 0) return LMGPU_OK;
  if (!index || !keys || !meas || (noise_kind != LMGPU_N_UNIT && !noise)) {
    tr->err = std::string(who) + ": null array";
    return LMGPU_INVALID;
  }
  const int nl = factor_noise_doubles(kTranslationType, noise_kind);
  for (int i = 0; i < n; i++) {
    lmgpu_translation_recovery::Edge e{};
    e.index = index[i];
    e.k1 = keys[2 * i];
    e.k2 = keys[2 * i + 1];
    std::memcpy(e.z, meas + (size_t)i * 3, 3 * sizeof(double));
    e.noise_kind = noise_kind;
    if (nl) std::memcpy(e.noise, noise + (size_t)i * nl, nl * sizeof(double));
    e.robust = robust_kind;
    e.rk = robust_k;
    to.push_back(e);
  }
  if (tr->finalized) tr_release(tr);  // the input changed: the next finalize rebuilds
  return LMGPU_OK;
}

// the factors of `es` as buckets, one per (noise kind, robust kind, k), graph indices gi0 + position in es
int tr_add_buckets(lmgpu_translation_recovery* tr, int type, const std::vector<lmgpu_translation_recovery::Edge>& es, int gi0,
                   const std::map<uint64_t, int>& slot_of) {
  std::vector<char> done(es.size(), 0);
  for (size_t a = 0; a < es.size(); a++) {
    if (done[a]) continue;
    const int kind = es[a].noise_kind, nl = factor_noise_doubles(type, kind);
    std::vector<int32_t> gi, slots;
    std::vector<double> meas, noise;
    for (size_t i = a; i < es.size(); i++) {
      if (done[i] || es[i].noise_kind != kind || es[i].robust != es[a].robust || es[i].rk != es[a].rk) continue;
      done[i] = 1;
      gi.push_back(gi0 + (int)i);
      slots.push_back(slot_of.at(es[i].k1));
      slots.push_back(slot_of.at(es[i].k2));
      meas.insert(meas.end(), es[i].z, es[i].z + 3);
      noise.insert(noise.end(), es[i].noise, es[i].noise + nl);
    }
    const int rc = add_internal_factor_bucket(tr->h, type, (int)gi.size(), gi.data(), slots.data(), meas.data(), kind, nl ? noise.data() : nullptr,
                                              es[a].robust, es[a].rk);
    if (rc) return tr_inner(tr, rc);
  }
  return LMGPU_OK;
}

}  // namespace

extern "C" {

int lmgpu_translation_recovery_create(const lmgpu_config* cfg, lmgpu_translation_recovery** out) {
  if (!cfg || !out || cfg->world_size > 1) return LMGPU_INVALID;  // multi-rank is out of scope; device < 0: host logic only, run refuses
  lmgpu_translation_recovery* tr = new lmgpu_translation_recovery();
  tr->cfg = *cfg;
  tr->cfg.rank = 0;
  tr->cfg.world_size = 1;
  tr->cfg.flags = 0;
  *out = tr;
  return LMGPU_OK;
}

int lmgpu_translation_recovery_destroy(lmgpu_translation_recovery* tr) {
  if (!tr) return LMGPU_INVALID;
  tr_release(tr);
  delete tr;
  return LMGPU_OK;
}

const char* lmgpu_translation_recovery_last_error(const lmgpu_translation_recovery* tr) { return tr ? tr->err.c_str() : "null object"; }

int lmgpu_translation_recovery_seed(lmgpu_translation_recovery* tr, uint32_t seed) {
  if (!tr) return LMGPU_INVALID;
  tr->rng.seed(seed);
  return LMGPU_OK;
}

int lmgpu_translation_recovery_set_prior_sigma(lmgpu_translation_recovery* tr, double sigma) {
  if (!tr) return LMGPU_INVALID;
  if (!(sigma > 0.0)) {
    tr->err = "lmgpu_translation_recovery_set_prior_sigma: refused (!(sigma > 0))";
    return LMGPU_INVALID;
  }
  tr->prior_sigma = sigma;
  if (tr->finalized) tr_release(tr);
  return LMGPU_OK;
}

int lmgpu_translation_recovery_add_directions(lmgpu_translation_recovery* tr, int32_t n, const int32_t* index, const uint64_t* keys, const double* dirs,
                                              int32_t noise_kind, const double* noise, int32_t robust_kind, double robust_k) {
  if (!tr) return LMGPU_INVALID;
  return tr_add(tr, tr->dirs, "lmgpu_translation_recovery_add_directions", n, index, keys, dirs, noise_kind, noise, robust_kind, robust_k);
}

int lmgpu_translation_recovery_add_betweens(lmgpu_translation_recovery* tr, int32_t n, const int32_t* index, const uint64_t* keys, const double* meas,
                                            int32_t noise_kind, const double* noise, int32_t robust_kind, double robust_k) {
  if (!tr) return LMGPU_INVALID;
  return tr_add(tr, tr->betw, "lmgpu_translation_recovery_add_betweens", n, index, keys, meas, noise_kind, noise, robust_kind, robust_k);
}

int lmgpu_translation_recovery_finalize(lmgpu_translation_recovery* tr, double scale, int32_t n_init, const uint64_t* init_keys, const double* init_vals,
                                        int32_t n_order, const uint64_t* ordering) {
  if (!tr) return LMGPU_INVALID;
  typedef lmgpu_translation_recovery::Edge Edge;
  if (n_init < 0 || (n_init > 0 && (!init_keys || !init_vals)) || n_order < 0 || (n_order > 0 && !ordering)) {
    tr->err = "lmgpu_translation_recovery_finalize: bad initial values or ordering arrays";
    return LMGPU_INVALID;
  }
  // ---- host logic first: a refusal here changes nothing.  (A failure further down, while the inner handle is built, leaves the session
  // unfinalized; the generator moves on only when finalize succeeds.)
  auto by_index = [](const Edge& a, const Edge& b) { return a.index < b.index; };
  std::vector<Edge> dirs = tr->dirs, betw = tr->betw;
  std::stable_sort(dirs.begin(), dirs.end(), by_index);
  std::stable_sort(betw.begin(), betw.end(), by_index);
  for (const std::vector<Edge>* v : {&dirs, &betw})
    for (size_t i = 1; i < v->size(); i++)
      if ((*v)[i].index == (*v)[i - 1].index) {
        tr->err = "lmgpu_translation_recovery_finalize: duplicate index";
        return LMGPU_INVALID;
      }
  // getSameTranslationDSFMap (:49-60): sets of nodes joined by zero-direction edges -- measured().equals(Unit3(0, 0, 0)), every component
  // within Unit3::equals' default 1e-9 of zero; the representative is the smallest key of a set
  std::vector<uint64_t> keys;
  std::map<uint64_t, uint64_t> parent;
  auto see = [&](uint64_t k) {
    if (parent.emplace(k, k).second) keys.push_back(k);
  };
  auto find = [&](uint64_t k) {
    uint64_t r = k;
    while (parent.at(r) != r) r = parent.at(r);
    while (parent.at(k) != r) {
      const uint64_t nx = parent.at(k);
      parent[k] = r;
      k = nx;
    }
    return r;
  };
  for (const Edge& e : dirs) {
    see(e.k1);
    see(e.k2);
    const uint64_t a = find(e.k1), b = find(e.k2);
    const bool zero = std::fabs(e.z[0]) <= 1e-9 && std::fabs(e.z[1]) <= 1e-9 && std::fabs(e.z[2]) <= 1e-9;
    if (a != b && zero) parent[std::max(a, b)] = std::min(a, b);
  }
  const size_t n_dir_keys = keys.size();
  for (const Edge& e : betw) {
    see(e.k1);
    see(e.k2);
  }
  // removeSameTranslationNodes (:64-76)
  auto reduce = [&](const std::vector<Edge>& in) {
    std::vector<Edge> out;
    for (Edge e : in) {
      e.k1 = find(e.k1);
      e.k2 = find(e.k2);
      if (e.k1 != e.k2) out.push_back(e);
    }
    return out;
  };
  const std::vector<Edge> D = reduce(dirs), B = reduce(betw);
  // initializeRandomly's order of first appearance (:164-173)
  std::vector<uint64_t> vars;
  std::set<uint64_t> seen;
  for (const std::vector<Edge>* v : {&D, &B})
    for (const Edge& e : *v)
      for (uint64_t k : {e.k1, e.k2})
        if (seen.insert(k).second) vars.push_back(k);
  const bool zero_only = vars.empty() && n_dir_keys > 0;  // :218-223: every set's representative at the origin
  if (zero_only)
    for (size_t i = 0; i < n_dir_keys; i++)
      if (find(keys[i]) == keys[i]) {
        vars.push_back(keys[i]);
        seen.insert(keys[i]);
      }
  // addSameTranslationNodes (:80-97) reads the representative's result: a set none of whose edges remains has none.  A key that is alone
  // in its set and still has no value appears only in between-translations that were dropped (both ends the same node): the reference
  // would return no value for it
  {
    std::map<uint64_t, int> set_size;
    for (uint64_t k : keys) set_size[find(k)]++;
    for (uint64_t k : keys)
      if (!seen.count(find(k))) {
        tr->err = set_size.at(find(k)) > 1
                      ? "lmgpu_translation_recovery_finalize: a set of nodes merged by zero-direction edges has no other edge left"
                      : "lmgpu_translation_recovery_finalize: a key appears only in between-translations whose two ends are the same node";
        return LMGPU_INVALID;
      }
  }
  // the ordering: a boundary input over the original keys, non-representatives ignored; default = first appearance
  std::vector<uint64_t> slot_keys;
  if (n_order > 0) {
    std::set<uint64_t> in_order;
    for (int i = 0; i < n_order; i++) {
      if (!in_order.insert(ordering[i]).second) {
        tr->err = "lmgpu_translation_recovery_finalize: duplicate key in the ordering";
        return LMGPU_INVALID;
      }
      if (seen.count(ordering[i])) slot_keys.push_back(ordering[i]);
    }
    if (slot_keys.size() != vars.size()) {
      tr->err = "lmgpu_translation_recovery_finalize: a variable is not in the ordering";
      return LMGPU_INVALID;
    }
  } else {
    slot_keys = vars;
  }
  std::map<uint64_t, int> slot_of;
  for (size_t s = 0; s < slot_keys.size(); s++) slot_of[slot_keys[s]] = (int)s;
  // ---- build
  tr_release(tr);
  std::map<uint64_t, const double*> given;
  for (int i = 0; i < n_init; i++) given.emplace(init_keys[i], init_vals + (size_t)i * 3);
  std::vector<double> initial(3 * slot_keys.size(), 0.0);
  std::mt19937 rng = tr->rng;  // drawn from a copy, handed back on success
  if (!zero_only)
    for (uint64_t k : vars) {
      double* v = &initial[3 * (size_t)slot_of.at(k)];
      auto it = given.find(k);
      for (int c = 0; c < 3; c++) v[c] = it != given.end() ? it->second[c] : tr_uniform(rng);
    }
  tr->keys = keys;
  tr->rep.resize(keys.size());
  for (size_t i = 0; i < keys.size(); i++) tr->rep[i] = find(keys[i]);
  tr->slot_keys = slot_keys;
  tr->initial = initial;
  tr->n_dir = (int)D.size();
  tr->n_fac = 0;
  if (!D.empty()) {  // buildGraph (:99-117) + addPrior (:119-143); without a direction edge addPrior returns at once and the graph is empty
    int rc;
    auto fail = [&](int code) {
      const std::string keep = tr->err;
      tr_release(tr);
      tr->err = keep;
      return code;
    };
    if ((rc = lmgpu_create(&tr->cfg, &tr->h))) {
      tr->err = "lmgpu_translation_recovery_finalize: lmgpu_create failed";
      return rc;
    }
    const int ns = (int)slot_keys.size(), m = (int)D.size();
    std::vector<int32_t> types(ns, LMGPU_POINT3);
    if ((rc = tr_inner(tr, lmgpu_set_variables(tr->h, ns, slot_keys.data(), types.data())))) return fail(rc);
    if ((rc = tr_add_buckets(tr, kTranslationType, D, 0, slot_of))) return fail(rc);
    {
      const int32_t gi = m, slot = slot_of.at(D[0].k1);
      const double zero[3] = {0, 0, 0}, inv[3] = {1.0 / tr->prior_sigma, 1.0 / tr->prior_sigma, 1.0 / tr->prior_sigma};
      if ((rc = tr_inner(tr, lmgpu_add_factor_bucket(tr->h, LMGPU_F_PRIOR_POINT3, 1, &gi, &slot, zero, LMGPU_N_DIAG, inv)))) return fail(rc);
    }
    tr->n_fac = m + 1;
    if (B.empty()) {
      const int32_t gi = m + 1, slot = slot_of.at(D[0].k2);
      const double z[3] = {scale * D[0].z[0], scale * D[0].z[1], scale * D[0].z[2]};
      if ((rc = tr_inner(tr, lmgpu_add_factor_bucket_robust(tr->h, LMGPU_F_PRIOR_POINT3, 1, &gi, &slot, z, D[0].noise_kind,
                                                            D[0].noise_kind != LMGPU_N_UNIT ? D[0].noise : nullptr, D[0].robust, D[0].rk))))
        return fail(rc);
      tr->n_fac += 1;
    } else {
      if ((rc = tr_add_buckets(tr, kBetweenPoint3Type, B, m + 1, slot_of))) return fail(rc);
      tr->n_fac += (int)B.size();
    }
    if ((rc = tr_inner(tr, lmgpu_finalize_structure(tr->h)))) return fail(rc);
    if (tr->cfg.device >= 0 && (rc = tr_inner(tr, lmgpu_set_values(tr->h, initial.data())))) return fail(rc);
  }
  tr->rng = rng;
  tr->finalized = true;
  return LMGPU_OK;
}

int lmgpu_translation_recovery_num_keys(const lmgpu_translation_recovery* tr) { return (tr && tr->finalized) ? (int)tr->keys.size() : -1; }
int lmgpu_translation_recovery_num_factors(const lmgpu_translation_recovery* tr) { return (tr && tr->finalized) ? tr->n_fac : -1; }
int lmgpu_translation_recovery_get_keys(const lmgpu_translation_recovery* tr, uint64_t* keys_out, uint64_t* representative_out) {
  if (!tr || !tr->finalized) return -1;
  if (keys_out) std::memcpy(keys_out, tr->keys.data(), tr->keys.size() * sizeof(uint64_t));
  if (representative_out) std::memcpy(representative_out, tr->rep.data(), tr->rep.size() * sizeof(uint64_t));
  return (int)tr->keys.size();
}
int lmgpu_translation_recovery_get_slots(const lmgpu_translation_recovery* tr, uint64_t* keys_out) {
  if (!tr || !tr->finalized) return -1;
  if (keys_out) std::memcpy(keys_out, tr->slot_keys.data(), tr->slot_keys.size() * sizeof(uint64_t));
  return (int)tr->slot_keys.size();
}
int lmgpu_translation_recovery_get_initial(const lmgpu_translation_recovery* tr, double* out) {
  if (!tr || !tr->finalized || !out) return LMGPU_INVALID;
  std::memcpy(out, tr->initial.data(), tr->initial.size() * sizeof(double));
  return LMGPU_OK;
}
lmgpu_handle* lmgpu_translation_recovery_handle(lmgpu_translation_recovery* tr) { return (tr && tr->finalized) ? tr->h : nullptr; }

int lmgpu_translation_recovery_run(lmgpu_translation_recovery* tr, const lmgpu_lm_params* p, lmgpu_lm_state* state_out) {
  if (!tr) return LMGPU_INVALID;
  if (!tr->finalized || !p) {
    tr->err = "lmgpu_translation_recovery_run: refused (lmgpu_translation_recovery_finalize has not succeeded, or no parameters)";
    return LMGPU_INVALID;
  }
  if (tr->cfg.device < 0) {
    tr->err = "lmgpu_translation_recovery_run: refused (the session was created without a device)";
    return LMGPU_HIP_ERROR;
  }
  std::vector<double> sol = tr->initial;  // an empty graph: LevenbergMarquardtOptimizer returns its initial values
  lmgpu_lm_state st{};
  if (tr->h) {
    if (tr->h->solver == LMGPU_SOLVER_PCG) {
      tr->err = "lmgpu_translation_recovery_run: refused (PCG on the inner handle; TranslationRecovery solves with the direct solver)";
      return LMGPU_INVALID;
    }
    int rc;
    if ((rc = tr_inner(tr, lmgpu_set_values(tr->h, tr->initial.data())))) return rc;
    if ((rc = tr_inner(tr, lmgpu_lm_init(tr->h, p, &st)))) return rc;
    rc = tr_inner(tr, lmgpu_optimize(tr->h, p, &st));
    if (state_out) *state_out = st;
    if (rc) return rc;
    if ((rc = tr_inner(tr, lmgpu_get_values(tr->h, sol.data())))) return rc;
  } else if (state_out) {
    *state_out = st;
  }
  // addSameTranslationNodes (:80-97): a merged-away node receives its representative's value
  std::map<uint64_t, int> slot_of;
  for (size_t s = 0; s < tr->slot_keys.size(); s++) slot_of[tr->slot_keys[s]] = (int)s;
  tr->result.assign(3 * tr->keys.size(), 0.0);
  for (size_t i = 0; i < tr->keys.size(); i++) std::memcpy(&tr->result[3 * i], &sol[3 * (size_t)slot_of.at(tr->rep[i])], 3 * sizeof(double));
  tr->have_result = true;
  return LMGPU_OK;
}

int lmgpu_translation_recovery_get(const lmgpu_translation_recovery* tr, double* out) {
  if (!tr || !tr->finalized || !tr->have_result || !out) return LMGPU_INVALID;
  std::memcpy(out, tr->result.data(), tr->result.size() * sizeof(double));
  return LMGPU_OK;
}

}  // extern "C"
