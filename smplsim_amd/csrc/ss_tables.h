// ss_tables.h — host-side construction of the index/constant tables the wavefront kernel uses.
//
// One environment is stepped by one 64-lane wavefront.  The kernel works on "nodes": node 0 = the
// root's 3 translational dofs, node 1 = its 3 rotational dofs, node b+1 = the 3 hinges of body b,
// so dof d belongs to node d/3.  Every node is a 3-dof joint of an articulated-body recursion: node 0
// carries a massless virtual body, node b+1 carries body b.  The joint-space matrices (mass matrix,
// Newton Hessian M + J^T D J, Stable-PD matrix M + Kd dt) are never formed: systems with them are solved
// by the articulated-body sweeps of ss_kernel.h (aba_solve), level by level over this node tree.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/smplsim_hip.h"
#include "ss_hdr.h"

namespace ss {

// A model ready for upload: the headers the kernels get by value and the six device tables.
struct HostModel {
  Hdr h{}, h_sc{};                // h_sc: the same header on the plain (non-aliased) LDS layout: what body-body-contact batches run on (= h when h is not aliased)
  HdrC hc{};                      // centred elimination tree of the plain solves
  HdrSC sc{};
  uint64_t illegal_mask = 0;      // bodies whose floor contact terminates the episode
  double meaninertia = 0;         // mjModel.stat.meaninertia (scale of the solver's termination test); shape 0's
  std::string self_collision_unavailable;   // non-empty: the model cannot run with ss_env_cfg.self_collision (reason)
  std::vector<uint32_t> shared;   // tables copied into LDS once per workgroup: integer tables, then the real-valued ones
  std::vector<uint32_t> chainrec; // chain records (ss_hdr.h): uploaded behind the blob, copied into LDS behind its prefix
  std::vector<int32_t> candb;     // [ncand] body of each candidate, bit 8: capsule
  // one block per body shape: [nb][kBodyC] off3 ipos3 mass Ibody6 invw_tr (loaded into registers; several shapes: + the dof inverse weights,
  // shape_stride), [ncand][kCandC], [nb][kGeomC] geoms in their body frames (pair functions of the SELFCOL kernels)
  std::vector<real> bodyc, candc, geomc;
  std::vector<int32_t> pairs;     // body-body candidate pairs after MuJoCo's static filters, 2 words each: b1 | b2 << 8 (normal points b1 -> b2), and the float
                                  // bits of the pair's bounding-sphere reach r1 + r2 + margin (broad phase); behind the last shape's: sc.o_sctab
};
struct Tree {   // everything that follows from body_parent alone
  std::vector<int> parent, chainnode, ndepth; int nlev = 0;    // node_tree
  std::vector<uint32_t> chainrec;                              // chain_records
  std::vector<int> sum_small, sum_big, sum_cover;              // subtree_sum_tables
  HdrC hc{}; int maxlev = 1;                                   // elimination_tree (hc.o_lev: assemble_blob); maxlev = its widest level
  std::vector<int> levrec, towards, joint, negated;            //   the level records of HdrC::o_lev; per body: neighbour towards the root (255: it is the root), joint node, S negated
};
// What the body shapes of one model must agree in (same_topology).  h: dims, candidate counts and physics scalars; the rest of it is filled in once per model.
struct Topology {
  Hdr h{};
  Tree tree;
  std::vector<real> dofc;         // [nv][kDofC]: arm, lo, hi, limited, invw (left 0: Shape::invw), kp, kd, tlim, ascale, aoffset, actuated, actuator index
  std::vector<int32_t> candb, pair_ids;
  uint64_t illegal_mask = 0;
};
struct Shape {   // what they may differ in
  std::vector<real> bodyc, invw, boff, candc, geomc;           // invw [nv] dof inverse weights, boff [nb][3] body frame offsets in the parent frame (chain walk of forward_kin)
  std::vector<int32_t> reach;                                  // float bits of the bounding-sphere reach per pair of Topology::pair_ids
  double meaninertia = 0;
};

inline void quat2mat(const double *q, double *m) {
  double w = q[0], x = q[1], y = q[2], z = q[3];
  double n = std::sqrt(w * w + x * x + y * y + z * z);
  w /= n; x /= n; y /= n; z /= n;
  m[0] = 1 - 2 * (y * y + z * z); m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = 1 - 2 * (x * x + z * z); m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = 1 - 2 * (x * x + y * y);
}
// inertia of body b in its body frame: R diag(I) R^T, R = the inertial frame's orientation
inline void body_frame_inertia(const ss_model_desc &d, int b, double *I) {
  double R[9]; quat2mat(d.body_iquat + 4 * b, R);
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
    double s = 0; for (int k = 0; k < 3; k++) s += R[3 * i + k] * d.body_inertia[3 * b + k] * R[3 * j + k];
    I[3 * i + j] = s;
  }
}

// mean diagonal of the joint-space inertia matrix at qpos0 (armature included) = mjModel.stat.meaninertia.  At qpos0 every body frame of
// these humanoids is aligned with the world (hinges at zero, root orientation identity), so dof (body j, axis a) sees
//     M_ii = sum over the bodies b of j's subtree of  a^T I_b a + m_b |a x (c_b - p_j)|^2   (+ armature),
// and the free joint the total mass (3 x) and the same sum about the root's position (3 x).
// (ss_model_desc has neither body quaternions nor joint axes: every model it can describe has world-aligned body frames at
// the zero pose and three hinges x, y, z per body, which is what the sums below use; the root orientation in qpos0 does not enter —
// the diagonal of M is invariant under a rigid rotation of the whole tree, the root's angular dofs being body-frame ones.)
inline double meaninertia_at_qpos0(const ss_model_desc &d) {
  const int nb = d.nbody, nv = 6 + 3 * (nb - 1);
  std::vector<double> p(3 * nb), c(3 * nb), I(9 * nb);
  for (int b = 0; b < nb; b++) {
    for (int k = 0; k < 3; k++) p[3 * b + k] = b == 0 ? d.qpos0[k] : p[3 * d.body_parent[b] + k] + d.body_pos[3 * b + k];
    for (int k = 0; k < 3; k++) c[3 * b + k] = p[3 * b + k] + d.body_ipos[3 * b + k];
    body_frame_inertia(d, b, &I[9 * b]);
  }
  double trace = 0;
  for (int j = 0; j < nb; j++)
    for (int a = 0; a < 3; a++) {
      double s = d.dof_armature[j == 0 ? 3 + a : 6 + 3 * (j - 1) + a];
      for (int b = j; b < nb; b++) {
        int t = b; while (t > j) t = d.body_parent[t];
        if (t != j) continue;                                // b is not in j's subtree
        const double r[3] = {c[3 * b] - p[3 * j], c[3 * b + 1] - p[3 * j + 1], c[3 * b + 2] - p[3 * j + 2]};
        const double r2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
        s += I[9 * b + 4 * a] + d.body_mass[b] * (r2 - r[a] * r[a]);
        if (j == 0 && a == 0) trace += 3 * d.body_mass[b];   // the three translational dofs
      }
      trace += s;
    }
  for (int a = 0; a < 3; a++) trace += d.dof_armature[a];
  return trace / (nv > 1 ? nv : 1);
}

// ---- The stages of build_host_model (at the end).  One that can refuse the description returns the message, or null.
// Every check that needs no table.
inline const char *validate(const ss_model_desc &d) {
  const int nb = d.nbody, nv = 6 + 3 * (nb - 1);
  if (nb < 1 || nb > 63) return "nbody must be in [1,63]";
  if (d.body_parent[0] != -1) return "body 0 must be the root";
  for (int b = 1; b < nb; b++) if (d.body_parent[b] < 0 || d.body_parent[b] >= b) return "parents must precede children";
  // bodies must come in depth-first order (the subtree of b is the index range [b, b + size): subtree_sum_tables): b's parent is
  // b - 1 or one of its ancestors
  for (int b = 2; b < nb; b++) {
    int a = b - 1;
    while (a > 0 && a != d.body_parent[b]) a = d.body_parent[a];
    if (a != d.body_parent[b]) return "bodies must be in depth-first order";
  }
  // (the root solve treats the free joint as a plain 6x6 system)
  for (int i = 0; i < 6; i++) if (d.dof_armature[i] != 0.0) return "armature on the free joint is not supported";
  std::vector<bool> driven(nv, false);
  for (int i = 0; i < d.nu; i++) {
    const int dof = d.actuator_dof[i];
    if (dof < 6 || dof >= nv || driven[dof]) return "bad actuator_dof";
    driven[dof] = true;
  }
  for (int b = 0; b < nb; b++) if (d.geom_type[b] != SS_GEOM_BOX && d.geom_type[b] != SS_GEOM_CAPSULE && d.geom_type[b] != SS_GEOM_SPHERE) return "unknown geom type";
  if (d.impratio != 1.0) return "impratio != 1 is not supported";
  return nullptr;
}

// Node tree (node b + 1 = body b below the two nodes of the free joint) and every node's chain from the root, itself included at its depth.
inline const char *node_tree(Tree &t) {
  const int nb = (int)t.parent.size(), nn = nb + 1;
  std::vector<int> nparent(nn); t.ndepth.assign(nn, 0);
  nparent[0] = -1; nparent[1] = 0; t.ndepth[1] = 1;
  for (int b = 1; b < nb; b++) { nparent[b + 1] = t.parent[b] + 1; t.ndepth[b + 1] = t.ndepth[t.parent[b] + 1] + 1; }
  t.nlev = 1 + *std::max_element(t.ndepth.begin(), t.ndepth.end());
  if (t.nlev > 32) return "tree too deep";
  t.chainnode.assign(nn * t.nlev, 0);                      // row width: the number of levels
  for (int n = 0; n < nn; n++)
    for (int a = n; a >= 0; a = nparent[a]) t.chainnode[n * t.nlev + t.ndepth[a]] = a;
  return nullptr;
}

// The chain records of ss_hdr.h from the node tree: per node chain_rec_bytes(nlev) bytes, four to a 32-bit word, lowest first — the node's
// depth, then per level k the node chainnode[n][k] for k <= depth and the node itself behind it (a reader that clamps nothing reads
// a valid row there and selects it away).
inline void chain_records(Tree &t) {
  const int nn = (int)t.ndepth.size(), nby = chain_rec_bytes(t.nlev);
  t.chainrec.assign((size_t)chain_rec_words(nn, t.nlev), 0u);
  auto put = [&](int n, int i, uint32_t v) { t.chainrec[(size_t)n * (nby / 4) + i / 4] |= v << (8 * (i & 3)); };
  for (int n = 0; n < nn; n++) {
    put(n, 0, (uint32_t)t.ndepth[n]);
    for (int k = 0; k + 1 < nby; k++) put(n, 1 + k, (uint32_t)(k <= t.ndepth[n] ? t.chainnode[n * t.nlev + k] : n));
  }
}

// Subtree sums in two phases (ss_kernel.h subtree_sum).  Bodies are in depth-first order, so the subtree of b is the index range
// [b, b + size).  Bodies whose subtree has <= 8 bodies sum their index range directly (one trip of 8 reads); the few large ones add
// their own value, the finished sums of their small children and, recursively, the terms of their large children ("cover": index
// t < 64 = input of body t, t >= 64 = phase-1 output of body t - 64; at most 63 entries per body, 63 x 63 < 4096 in all: the fields of sum_big hold them).
inline void subtree_sum_tables(Tree &t) {
  const int nb = (int)t.parent.size(), kSmall = 8;
  std::vector<int> subsize(nb, 1), order(nb);
  for (int b = nb - 1; b >= 1; b--) subsize[t.parent[b]] += subsize[b];
  for (int b = 0; b < nb; b++) order[b] = b;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return subsize[x] > subsize[y]; });
  std::vector<std::vector<int>> cov(nb);
  for (int b = nb - 1; b >= 0; b--) {                        // children before parents (depth-first order)
    if (subsize[b] <= kSmall) continue;
    cov[b].push_back(b);
    for (int c = b + 1; c < nb; c++) {
      if (t.parent[c] != b) continue;
      if (subsize[c] <= kSmall) cov[b].push_back(64 + c);
      else cov[b].insert(cov[b].end(), cov[c].begin(), cov[c].end());
    }
  }
  for (int b : order) {
    if (subsize[b] <= kSmall) { t.sum_small.push_back(b | (subsize[b] << 8)); continue; }
    t.sum_big.push_back(b | ((int)t.sum_cover.size() << 8) | ((int)cov[b].size() << 20));
    t.sum_cover.insert(t.sum_cover.end(), cov[b].begin(), cov[b].end());
  }
}

// Elimination tree of the articulated-body sweeps (HdrC): the body tree re-rooted at its centre.  The root minimises the depth (ties:
// the narrower widest level, then the lower index); the widest level may not exceed 16 nodes (two passes of 8 lane groups).
// Picks the root and gives every body its level (dep) and its neighbour towards the root (tw, -1 for the root).
inline int centre_of_tree(const Tree &t, std::vector<int> &dep, std::vector<int> &tw) {
  const int nb = (int)t.parent.size();
  std::vector<std::vector<int>> adj(nb);
  for (int b = 1; b < nb; b++) { adj[b].push_back(t.parent[b]); adj[t.parent[b]].push_back(b); }
  auto bfs = [&](int c) {
    dep.assign(nb, -1); tw.assign(nb, -1);
    std::vector<int> q{c}; dep[c] = 0;
    for (size_t i = 0; i < q.size(); i++) for (int o : adj[q[i]]) if (dep[o] < 0) { dep[o] = dep[q[i]] + 1; tw[o] = q[i]; q.push_back(o); }
  };
  int best = 0, bestd = 1 << 30, bestw = 1 << 30;
  for (int c = 0; c < nb; c++) {
    bfs(c);
    const int dmax = *std::max_element(dep.begin(), dep.end());
    std::vector<int> wd(dmax + 1, 0); for (int b = 0; b < nb; b++) wd[dep[b]]++;
    const int wmax = dmax ? *std::max_element(wd.begin() + 1, wd.end()) : 0;
    if (wmax > 16) continue;
    if (dmax < bestd || (dmax == bestd && wmax < bestw)) { best = c; bestd = dmax; bestw = wmax; }
  }
  bfs(best);
  return best;
}
// Level lists: children of one node contiguous, in the order of their parents' positions; a node's children by falling height of
// their subtrees (ties: body index) — the limbs' nodes then keep one slot from level to level and the leaves come last, which is
// what lets the sweep towards the root keep a limb's rows in registers (hc.chain)
inline std::vector<std::vector<int>> level_lists(int root, int nlev, const std::vector<int> &dep, const std::vector<int> &tw) {
  const int nb = (int)dep.size();
  std::vector<int> hgt(nb, 0);
  for (int L = nlev; L >= 1; L--) for (int b = 0; b < nb; b++) if (dep[b] == L) hgt[tw[b]] = std::max(hgt[tw[b]], hgt[b] + 1);
  std::vector<std::vector<int>> levb(nlev + 1);
  levb[0].push_back(root);
  for (int L = 1; L <= nlev; L++)
    for (int pb : levb[L - 1]) {
      std::vector<int> ch;
      for (int b = 0; b < nb; b++) if (dep[b] == L && tw[b] == pb) ch.push_back(b);
      std::stable_sort(ch.begin(), ch.end(), [&](int x, int y) { return hgt[x] > hgt[y]; });
      levb[L].insert(levb[L].end(), ch.begin(), ch.end());
    }
  return levb;
}
// The level records and packed level properties of HdrC for that root, and the same per body (towards, joint, negated).
inline const char *elimination_tree(Tree &t) {
  const int nb = (int)t.parent.size();
  std::vector<int> dep, tw;
  HdrC &hc = t.hc;
  hc.root = centre_of_tree(t, dep, tw);
  hc.nlev = *std::max_element(dep.begin(), dep.end()); hc.pel_level = dep[0];
  const int nlev = hc.nlev;
  const std::vector<std::vector<int>> levb = level_lists(hc.root, nlev, dep, tw);
  t.towards.assign(nb, 255); t.joint.assign(nb, 0); t.negated.assign(nb, 0);
  int maxlev = 0; bool cpack_unrepresentable = false;
  for (int L = 1; L <= nlev; L++) {
    const int nk = (int)levb[L].size();
    maxlev = std::max(maxlev, nk);
    hc.nkpack[(L - 1) >> 4] |= (unsigned long long)(nk - 1) << (4 * ((L - 1) & 15));
    int cmaxL = 0, slot = 0;
    bool chainL = L < nlev;
    for (int b : levb[L]) {
      const int e = tw[b];                                    // neighbour towards the root
      const bool kin = t.parent[b] == e;                      // walked along the kinematic direction: b's own joint
      const int jn = (kin ? b : e) + 1;                       // node index of the joint on this edge (its dofs are 3 jn ..)
      int cfirst = 0, cc = 0;
      if (L < nlev)
        for (int k2 = 0; k2 < (int)levb[L + 1].size(); k2++)
          if (tw[levb[L + 1][k2]] == b) { if (cc == 0) cfirst = k2; cc++; }
      t.towards[b] = e; t.joint[b] = jn; t.negated[b] = kin ? 0 : 1;
      t.levrec.push_back(b | (jn << 8) | (e << 16) | ((kin ? 0 : 1) << 24) | ((b == 0 ? 1 : 0) << 25));
      t.levrec.push_back(cfirst | (cc << 8));
      if (!kin) hc.neg |= 1ull << (L - 1);
      cmaxL = std::max(cmaxL, cc);
      if (cc > 1 || (cc == 1 && cfirst != slot)) chainL = false;
      slot++;
    }
    if (chainL) hc.chain |= 1ull << (L - 1);
    // the fixed-layout instantiations read this as "most children of a node of level L" (3 bits per level): a tree with a node of
    // more than 7 children below the root, or deeper than 21 levels, gets a value no instantiation is built for (runtime kernel)
    if (L <= 21 && cmaxL <= 7) hc.cpack |= (unsigned long long)cmaxL << (3 * (L - 1));
    else cpack_unrepresentable = true;
  }
  if (t.levrec.empty()) t.levrec.assign(2, 0);
  if (cpack_unrepresentable) hc.cpack = ~0ull;
  if (maxlev > 16) return "more than 16 nodes in one tree level";
  t.maxlev = std::max(maxlev, 1);                            // sizes the level buffer of the LDS layout
  return nullptr;
}

// Dof constants, the inverse weight column left zero.
inline std::vector<real> dof_constants(const ss_model_desc &d) {
  const int nv = 6 + 3 * (d.nbody - 1);
  std::vector<int> dof_act(nv, -1);                         // actuator index of a dof or -1
  for (int i = 0; i < d.nu; i++) dof_act[d.actuator_dof[i]] = i;
  std::vector<real> dofc(nv * kDofC, real(0));
  for (int i = 0; i < nv; i++) {
    real *c = &dofc[i * kDofC];
    c[0] = (real)d.dof_armature[i]; c[1] = (real)d.jnt_range[2 * i]; c[2] = (real)d.jnt_range[2 * i + 1];
    c[3] = (i >= 6 && d.jnt_limited[i]) ? 1.f : 0.f;
    const int a = dof_act[i];
    if (a >= 0) {
      c[5] = (real)d.kp[a]; c[6] = (real)d.kd[a]; c[7] = (real)d.torque_lim[a];
      c[8] = (real)d.act_scale[a]; c[9] = (real)d.act_offset[a]; c[10] = 1.f; c[11] = (real)a;
    } else c[11] = -1.f;
  }
  return dofc;
}

// Body constants (registers): off3 ipos3 mass Ibody(xx xy xz yy yz zz) invw_tr; the dof inverse weights; the body offsets; meaninertia.
inline const char *body_constants(const ss_model_desc &d, Shape &s) {
  const int nb = d.nbody, nv = 6 + 3 * (nb - 1);
  // mjModel.stat.meaninertia; <= 0 (e.g. a caller of the pre-round-3 struct, zero-initialised): computed here from the description
  s.meaninertia = d.meaninertia > 0.0 ? d.meaninertia : meaninertia_at_qpos0(d);
  if (!(s.meaninertia > 0.0)) return "meaninertia: the inertia matrix at qpos0 has no positive diagonal";
  s.bodyc.assign(nb * kBodyC, real(0)); s.boff.assign(3 * nb, real(0));
  s.invw.assign(d.dof_invweight0, d.dof_invweight0 + nv);
  for (int b = 0; b < nb; b++) {
    real *c = &s.bodyc[b * kBodyC];
    // (the root's offset is its initial position, not a parent-frame offset: left zero)
    for (int k = 0; k < 3; k++) { c[k] = s.boff[3 * b + k] = b == 0 ? real(0) : (real)d.body_pos[3 * b + k]; c[3 + k] = (real)d.body_ipos[3 * b + k]; }
    c[6] = (real)d.body_mass[b];
    double I[9]; body_frame_inertia(d, b, I);
    c[7] = (real)I[0]; c[8] = (real)I[1]; c[9] = (real)I[2]; c[10] = (real)I[4]; c[11] = (real)I[5]; c[12] = (real)I[8];
    c[13] = (real)d.body_invweight0[2 * b];
  }
  return nullptr;
}

// Floor-contact candidates: boxes first (8 corners each, 8-aligned), then two per capsule or sphere; the counts that follow from them.
inline void floor_candidates(const ss_model_desc &d, Topology &t, Shape &s) {
  const int nb = d.nbody; Hdr &h = t.h;
  for (int b = 0; b < nb; b++) {
    if (d.geom_type[b] != SS_GEOM_BOX) continue;
    double G[9]; quat2mat(d.geom_quat + 4 * b, G);
    for (int i = 0; i < 8; i++) {
      const double *z = d.geom_size + 3 * b, v[3] = {(i & 1) ? z[0] : -z[0], (i & 2) ? z[1] : -z[1], (i & 4) ? z[2] : -z[2]};
      real c[kCandC] = {0};
      for (int r = 0; r < 3; r++) {
        c[r] = (real)(G[3 * r] * v[0] + G[3 * r + 1] * v[1] + G[3 * r + 2] * v[2]);    // corner vector (body frame)
        c[3 + r] = (real)d.geom_pos[3 * b + r];                                         // box centre (body frame)
      }
      c[7] = (real)d.body_invweight0[2 * b];
      s.candc.insert(s.candc.end(), c, c + kCandC); t.candb.push_back(b);
    }
    h.nbox++;
  }
  for (int b = 0; b < nb; b++) {
    if (d.geom_type[b] == SS_GEOM_BOX) continue;
    const bool sphere = d.geom_type[b] == SS_GEOM_SPHERE;    // a capsule of zero half length: ONE floor contact (mjc_PlaneSphere), no tangent hint
    double G[9]; quat2mat(d.geom_quat + 4 * b, G);
    for (int e = 0; e < 2; e++) {
      double sg = e ? -1.0 : 1.0;
      real c[kCandC] = {0};
      for (int r = 0; r < 3; r++) {
        c[r] = (real)(d.geom_pos[3 * b + r] + (sphere ? 0.0 : sg * G[3 * r + 2] * d.geom_size[3 * b + 1]));   // end-sphere centre (body frame)
        c[3 + r] = sphere ? real(0) : (real)G[3 * r + 2];                                    // capsule axis (body frame): the first tangent's hint
      }
      // (the slot pairing of the solver wants two candidates per non-box body: a sphere's second one has a radius that never qualifies)
      c[6] = (sphere && e == 1) ? real(-1e30) : (real)d.geom_size[3 * b];                    // radius
      c[7] = (real)d.body_invweight0[2 * b];
      s.candc.insert(s.candc.end(), c, c + kCandC); t.candb.push_back(b | 256);
    }
  }
  h.ncand = (int)t.candb.size();
  h.nslot = 4 * h.nbox + 2 * (nb - h.nbox);
  for (int b = 0; b < nb; b++)
    if (!(d.legal_contact && d.legal_contact[b])) t.illegal_mask |= 1ull << b;
}

// Body-body collision: candidate pairs (mj_collision's static filters: contype / conaffinity masks, parent-child filter, <exclude>
// pairs) and the geom table of the pair functions.  The pair's first geom is the one MuJoCo hands to the pair function first (the
// lower type id: sphere 2 < capsule 3 < box 6, then the lower geom id); contact normals point from it to the second.
inline void pair_and_geom_tables(const ss_model_desc &d, Topology &t, Shape &s) {
  const int nb = d.nbody;
  auto rank = [&](int b) { return d.geom_type[b] == SS_GEOM_SPHERE ? 0 : (d.geom_type[b] == SS_GEOM_CAPSULE ? 1 : 2); };
  // bounding spheres about the geom centres: half diagonal of a box, radius + half length of a capsule
  auto reach = [&](int b) {
    const double *z = d.geom_size + 3 * b;
    return d.geom_type[b] == SS_GEOM_BOX ? std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]) : z[0] + (d.geom_type[b] == SS_GEOM_SPHERE ? 0.0 : z[1]);
  };
  for (int i = 0; i < nb; i++) for (int j = i + 1; j < nb; j++) {
    const int ct1 = d.geom_contype ? d.geom_contype[i] : 1, ca1 = d.geom_conaffinity ? d.geom_conaffinity[i] : 1;
    const int ct2 = d.geom_contype ? d.geom_contype[j] : 1, ca2 = d.geom_conaffinity ? d.geom_conaffinity[j] : 1;
    if (!((ct1 & ca2) || (ct2 & ca1))) continue;
    if (d.body_parent[j] == i || d.body_parent[i] == j) continue;
    bool ex = false;
    for (int e = 0; e < d.nexclude; e++)
      ex |= (d.exclude[2 * e] == i && d.exclude[2 * e + 1] == j) || (d.exclude[2 * e] == j && d.exclude[2 * e + 1] == i);
    if (ex) continue;
    const int first = rank(j) < rank(i) ? j : i;
    t.pair_ids.push_back(first | ((first == i ? j : i) << 8));
    // a hair of slack so that the float rounding of the sum can never prune a pair the pair function would report (those are strictly inside)
    const float rs = (float)((reach(i) + reach(j) + d.margin) * (1.0 + 1e-5));
    int32_t bits; std::memcpy(&bits, &rs, 4);
    s.reach.push_back(bits);
  }
  s.geomc.assign((size_t)nb * kGeomC, real(0));
  for (int b = 0; b < nb; b++) {
    real *c = &s.geomc[(size_t)b * kGeomC];
    double G[9]; quat2mat(d.geom_quat + 4 * b, G);
    for (int k = 0; k < 3; k++) { c[k] = (real)d.geom_pos[3 * b + k]; c[3 + k] = (real)d.geom_size[3 * b + k]; }
    if (d.geom_type[b] == SS_GEOM_SPHERE) { c[4] = 0; c[5] = 0; }                                // half length 0 whatever the caller left there
    for (int k = 0; k < 9; k++) c[6 + k] = (real)G[k];
    c[15] = (real)d.geom_type[b];
  }
}

inline void physics_scalars(const ss_model_desc &d, Hdr &h) {
  h.dt = (real)d.timestep; h.grav = (real)d.gravity; h.margin = (real)d.margin; h.mu = (real)d.friction;
  for (int k = 0; k < 5; k++) h.solimp[k] = (real)d.solimp[k];
  const double dmax = d.solimp[1], tc = d.solref[0] < 2 * d.timestep ? 2 * d.timestep : d.solref[0];
  h.K = (real)(1.0 / (dmax * dmax * tc * tc * d.solref[1] * d.solref[1]));
  h.B = (real)(2.0 / (dmax * tc));
  for (int k = 0; k < 3; k++) h.qpos0_root[k] = (real)d.qpos0[k];
}

// One description as its two parts.  like: the topology of the model's shape 0, whose tree tables serve every shape with its parents.
inline const char *describe(const ss_model_desc &d, const Topology *like, Topology &t, Shape &s) {
  if (const char *e = validate(d)) return e;
  const int nb = d.nbody;
  Hdr &h = t.h;
  h.nb = nb; h.nn = nb + 1; h.nv = 6 + 3 * (nb - 1); h.nq = h.nv + 1; h.nu = d.nu;
  t.tree.parent.assign(d.body_parent, d.body_parent + nb);
  if (!like || like->tree.parent != t.tree.parent) {
    if (const char *e = node_tree(t.tree)) return e;
    chain_records(t.tree);
    subtree_sum_tables(t.tree);
    if (const char *e = elimination_tree(t.tree)) return e;
  }
  t.dofc = dof_constants(d);
  if (const char *e = body_constants(d, s)) return e;
  floor_candidates(d, t, s);
  pair_and_geom_tables(d, t, s);
  physics_scalars(d, h);
  return nullptr;
}

// Everything but the geometry must agree: tree, joints, limits, gains, actuators, geom types, contact set, options.  The tables are
// compared as the device gets them: rounded to `real`, bit for bit.
inline bool same_topology(const Topology &a, const Topology &b) {
  const Hdr &h = a.h, &g = b.h;
  return h.nb == g.nb && h.nu == g.nu && h.ncand == g.ncand && h.nbox == g.nbox && h.nslot == g.nslot && a.tree.parent == b.tree.parent &&
         a.dofc.size() == b.dofc.size() && !std::memcmp(a.dofc.data(), b.dofc.data(), a.dofc.size() * sizeof(real)) && a.candb == b.candb &&
         a.pair_ids == b.pair_ids && a.illegal_mask == b.illegal_mask && h.dt == g.dt && h.grav == g.grav && h.margin == g.margin && h.mu == g.mu &&
         h.K == g.K && h.B == g.B;
}

// The shared blob (copied into LDS once per workgroup) and its offsets in h and hc: the integer tables, then, 16-byte aligned, the real-valued ones — the
// dof constants and the body offsets, with the shape's inverse weights and offsets, or zeros for a model of several shapes (read per env from bodyc).
// lean (the SMPL-X size class, where LDS, not the register file, caps the resident envs; goes with the aliased layout of ss_hdr.h make_layout): the
// dof-constant table stays in global memory — 12 reals per dof = 7.6 KB of the workgroup's LDS for 52 bodies, read once or twice per mj_step per lane
// (limits, Stable PD: L1-resident), except the armature, which the Newton iteration reads and which keeps a column of its own in LDS.  Together with the
// action read from global memory that is a seventh resident env per CU.  The LDS copy of the blob is its prefix of h.shared_words words; the dof table lies behind it.
inline std::vector<uint32_t> assemble_blob(const Topology &t, const Shape *shape, bool lean, Hdr &h, HdrC &hc) {
  std::vector<uint32_t> S;
  auto push_i = [&](const std::vector<int> &v) { int o = (int)S.size(); S.insert(S.end(), v.begin(), v.end()); return o; };
  const Tree &tr = t.tree;
  h.o_chainnode = push_i(tr.chainnode); h.o_ndepth = push_i(tr.ndepth); h.o_bparent = push_i(tr.parent);
  h.o_sumsmall = push_i(tr.sum_small); h.o_sumbig = push_i(tr.sum_big); h.o_sumcover = push_i(tr.sum_cover);
  hc.o_lev = push_i(tr.levrec);
  while (S.size() % 4) S.push_back(0u);                     // reals start 16-byte aligned
  const int o_real = (int)S.size(), real0 = o_real / (int)(sizeof(real) / 4);   // kernel-side offsets count reals from the start of the blob
  std::vector<real> dofc = t.dofc, boff(3 * h.nb, real(0)), F;
  if (shape) { boff = shape->boff; for (int i = 0; i < h.nv; i++) dofc[i * kDofC + 4] = shape->invw[i]; }
  auto push_r = [&](const std::vector<real> &v) { int o = real0 + (int)F.size(); F.insert(F.end(), v.begin(), v.end()); return o; };
  int o_arm = 0;
  if (lean) {
    h.o_boff = push_r(boff);
    o_arm = real0 + (int)F.size(); for (int i = 0; i < h.nv; i++) F.push_back(dofc[i * kDofC]);
    while (F.size() % 4) F.push_back(real(0));
  } else {
    h.o_dofc = push_r(dofc); h.o_boff = push_r(boff);
  }
  h.shared_words = o_real + (int)F.size() * (int)(sizeof(real) / 4);   // what a workgroup copies into LDS (the whole blob unless lean)
  if (lean) h.o_dofc = push_r(dofc);
  h.arm_lean = (unsigned long long)(uint32_t)o_arm | ((unsigned long long)(lean ? 1 : 0) << 32);
  S.resize(o_real + F.size() * (sizeof(real) / 4));
  std::memcpy(S.data() + o_real, F.data(), F.size() * sizeof(real));
  return S;
}

// One more block of the per-shape tables.  shaped (a model of several shapes): the block of bodyc ends in the dof inverse weights (shape_stride).
inline void append_shape(const Topology &t, const Shape &s, bool shaped, HostModel &out) {
  out.bodyc.insert(out.bodyc.end(), s.bodyc.begin(), s.bodyc.end());
  if (shaped) { out.bodyc.insert(out.bodyc.end(), s.invw.begin(), s.invw.end()); out.bodyc.resize(out.bodyc.size() + (4 - s.invw.size() % 4) % 4, real(0)); }
  out.candc.insert(out.candc.end(), s.candc.begin(), s.candc.end());
  out.geomc.insert(out.geomc.end(), s.geomc.begin(), s.geomc.end());
  for (size_t i = 0; i < s.reach.size(); i++) { out.pairs.push_back(t.pair_ids[i]); out.pairs.push_back(s.reach[i]); }
}

// Per-env LDS layouts (floats) of h, h_sc (= h but for its layout) and sc.  The SMPL-X size class gets the aliased one when its records fit
// (ss_hdr.h make_layout); body-body-contact batches of such a model run on the plain one, whose Aown .. (W, y) stretch holds their dense system.
inline const char *lds_layouts(bool alias, HostModel &m) {
  const Layout plain = make_layout(m.h.nb, m.h.maxlev, false);
  if (13 * m.h.nslot > plain.l_Wst - plain.l_An) return "contact record buffer does not fit";
  m.h_sc = m.h; apply_layout(m.h_sc, plain);
  apply_layout(m.h, alias ? make_layout(m.h.nb, m.h.maxlev, true) : plain);
  m.sc = make_layout_sc(m.h.nb, plain.env_floats, plain.l_An);
  return nullptr;
}

// Body-body contacts: behind the pair table, per body of the elimination tree (SELFCOL kernels copy this into the env's LDS slice) neighbour
// towards the root (255: it is the root) | joint node << 8 | (S negated) << 16, and the mask of the bodies on its way to the root (itself
// included, the root not); and whether the model can have them.
inline void body_contact_tables(const Topology &top, HostModel &m) {
  const Tree &t = top.tree; const int nb = m.h.nb;
  m.sc.npair = (int)top.pair_ids.size(); m.sc.o_sctab = (int)m.pairs.size();
  for (int b = 0; b < nb; b++) {
    unsigned long long pm = 0ull;
    for (int a = b; a != t.hc.root; a = t.towards[a]) pm |= 1ull << a;
    m.pairs.push_back(t.towards[b] | (t.joint[b] << 8) | (t.negated[b] << 16));
    m.pairs.push_back((int32_t)(uint32_t)(pm & 0xFFFFFFFFull)); m.pairs.push_back((int32_t)(uint32_t)(pm >> 32));
  }
  if (nb < 2) m.self_collision_unavailable = "a single body has no body-body contacts";
  // the dense assembly keeps 12 reals per joint between a contact's two bodies (at most 2 x levels of them) in the 6 nb reals of gc + zb
  else if (8 * t.hc.nlev > 64) m.self_collision_unavailable = "elimination tree deeper than 8 levels (one lane per (joint, row) of a contact's joints)";
  else if (12 * 2 * t.hc.nlev > m.sc.l_tab - m.sc.l_gc) m.self_collision_unavailable = "tree too deep for its body count (body-body contacts need 4 x levels <= bodies)";
}

// The model of num_shapes descriptions of one humanoid with different body shapes (1: the plain case).  plain_layout: never the aliased
// LDS layout and the lean tables (SS_NO_ALIAS_LAYOUT).  Returns the message of a refusal, or "".
inline std::string build_host_model(const ss_model_desc *d, int num_shapes, bool plain_layout, HostModel &out) {
  Topology top; Shape first;                                // of shape 0
  for (int s = 0; s < num_shapes; s++) {
    Topology t; Shape sh;
    if (const char *e = describe(d[s], s ? &top : nullptr, t, sh)) return num_shapes > 1 ? "shape " + std::to_string(s) + ": " + e : std::string(e);
    if (s && !same_topology(t, top)) return "shape " + std::to_string(s) + " differs from shape 0 in more than its geometry";
    append_shape(t, sh, num_shapes > 1, out);
    if (s == 0) { top = std::move(t); first = std::move(sh); }
  }
  const Tree &tree = top.tree;
  Hdr &h = out.h = top.h;
  h.nlev = tree.nlev; h.maxlev = tree.maxlev; h.n_sumsmall = (int)tree.sum_small.size(); h.n_sumbig = (int)tree.sum_big.size();
  out.hc = tree.hc; out.chainrec = tree.chainrec; out.candb = top.candb; out.illegal_mask = top.illegal_mask; out.meaninertia = first.meaninertia;
  const bool alias = h.nb > 32 && alias_layout_fits(h.nb, h.maxlev, h.nslot) && !plain_layout;
  out.shared = assemble_blob(top, num_shapes == 1 ? &first : nullptr, alias, h, out.hc);
  if (const char *e = lds_layouts(alias, out)) return e;
  body_contact_tables(top, out);
  return "";
}

inline int obs_size(const Hdr &h, const ss_env_cfg &c) {
  int nd = 3 * (h.nb - 1);
  int n = (c.root_height_obs ? 1 : 0) + nd + (c.self_obs_v == 1 ? 6 * h.nb + 6 + nd : 12 * h.nb);
  if (c.task == SS_TASK_SPEED || c.task == SS_TASK_REACH) n += 3;
  if (c.task == SS_TASK_GETUP) n += 1;
  return n;
}

}  // namespace ss
