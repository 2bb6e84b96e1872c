// hdbscan.cpp — HDBSCAN's labels read off a spanning tree, on the host (gr_hdbscan_host).  Plain C++: no HIP, no context, no GPU.  The tree is the
// n^2 d part and is built on the device (mst.hip); everything read off its n - 1 edges is sequential tree work of O(n log n) and is done here.
// The rules are scikit-learn 1.7's HDBSCAN at its defaults (cluster_selection_method="eom", allow_single_cluster=False,
// cluster_selection_epsilon=0, no max_cluster_size); where the paper and scikit-learn differ, scikit-learn's behaviour is the definition.  They are
// stated in include/ganrev.h and restated in numpy in tests/hierarchy_paths.py.  Operation by operation (all fp64, every operation on its own):
//   hierarchy         the edges are merged in the order given: edge k joins the components of eu[k] (left) and ev[k] (right) into node n + k of
//                     size left + right, at height ew[k]; rows are the nodes 0 .. n - 1, the root is node 2 n - 2
//   lambda            1 / w, and +inf at w = 0
//   condensed tree    the nodes n + k in DESCENDING k (every node after its parent), skipping nodes inside a side that has fallen out.  The root
//                     is cluster 0, born at lambda 0.  A node of cluster c with sides of L and R rows, m = min_cluster_size:
//                       L >= m and R >= m   the left side becomes a new cluster, then the right one (numbered in the order made), born at lambda
//                       one side below m    its rows fall out of c at lambda; the other side goes on as c
//                       both below m        the rows of both fall out of c at lambda
//                     term(c, lambda, s) = (lambda - birth_c) * (double)s, and 0 where lambda == birth_c (so inf - inf never arises); one term per
//                     side that leaves c - a new cluster or the rows that fall out, s its row count - left before right:
//   stability_c       stability_c + term, from +0.0, in that order;  lambda_max_c = the largest lambda of c's terms
//   selection         the clusters in DESCENDING number (every cluster after its children), the root left out: S = stability_left +
//                     stability_right for a cluster with children; where S > stability_c the cluster is not selected and stability_c = S,
//                     else it is selected and no cluster below it is.  The root is never selected
//   label of a row    the selected cluster that the cluster it fell out of is, or lies under; -1 without one
//   prob of a row     q = min(lambda_row, lambda_max_C) / lambda_max_C for its selected cluster C, and 1 where q is not finite; 0 for a row of -1
//   cluster numbers   0, 1, ... in ascending order of the selected clusters' smallest member rows
#include <cmath>
#include <cstdint>
#include <limits>
#include <new>
#include <vector>

#include "ganrev.h"

namespace {

struct Hierarchy { std::vector<int32_t> left, right, size; };           // node n + k: its sides and its row count

int find_root(std::vector<int32_t>& up, int32_t a) {
  int32_t r = a;
  while (up[r] != r) r = up[r];
  while (up[a] != r) { const int32_t next = up[a]; up[a] = r; a = next; }
  return r;
}

}  // namespace

extern "C" int gr_hdbscan_host(const int32_t* eu, const int32_t* ev, const double* ew, int64_t n, int min_cluster_size, int32_t* labels, double* prob,
                               int32_t* n_clusters) {
  if (!eu || !ev || !ew || !labels || !prob || !n_clusters) return GR_ERR_INVALID;
  if (n < 2 || n > (int64_t)1 << 30) return GR_ERR_INVALID;
  if (min_cluster_size < 2 || min_cluster_size > n) return GR_ERR_INVALID;
  const int64_t m = n - 1;
  for (int64_t k = 0; k < m; ++k) {
    if (eu[k] < 0 || ev[k] >= n || eu[k] >= ev[k]) return GR_ERR_INVALID;            // 0 <= eu < ev < n
    if (!(ew[k] >= 0.0) || !std::isfinite(ew[k])) return GR_ERR_INVALID;
    if (k > 0 && ew[k] < ew[k - 1]) return GR_ERR_INVALID;
  }
  try {
    const double inf = std::numeric_limits<double>::infinity();
    // ---- the hierarchy, by a union-find over the edges in the order given
    Hierarchy h;
    h.left.resize(m); h.right.resize(m); h.size.resize(m);
    {
      std::vector<int32_t> up(n), node(n), count(n, 1);                // per union-find root: the hierarchy node it stands for, its rows
      for (int64_t i = 0; i < n; ++i) { up[i] = (int32_t)i; node[i] = (int32_t)i; }
      for (int64_t k = 0; k < m; ++k) {
        const int32_t a = find_root(up, eu[k]), b = find_root(up, ev[k]);
        if (a == b) return GR_ERR_INVALID;                               // the edge closes a cycle
        h.left[k] = node[a]; h.right[k] = node[b]; h.size[k] = count[a] + count[b];
        const int32_t keep = count[a] >= count[b] ? a : b, gone = keep == a ? b : a;
        up[gone] = keep; count[keep] = h.size[k]; node[keep] = (int32_t)(n + k);
      }
    }
    auto rows_of = [&](int32_t nd) { return nd < n ? 1 : h.size[nd - n]; };
    // ---- the condensed tree
    std::vector<int32_t> cluster_of(m, -1);                             // per internal node: the cluster it belongs to; -1: inside a fallen side
    std::vector<int32_t> parent{-1}, child_a{-1}, child_b{-1};          // per cluster
    std::vector<double> birth{0.0}, stability{0.0}, lambda_max{0.0};
    std::vector<int32_t> row_cluster(n, 0);
    std::vector<double> row_lambda(n, 0.0);
    std::vector<int32_t> stack;
    cluster_of[m - 1] = 0;
    auto term = [&](int32_t c, double lambda, int32_t s) {
      const double t = lambda == birth[c] ? 0.0 : (lambda - birth[c]) * (double)s;
      stability[c] = stability[c] + t;
      if (lambda > lambda_max[c]) lambda_max[c] = lambda;
    };
    auto fall_out = [&](int32_t nd, int32_t c, double lambda) {         // every row under nd leaves c at lambda
      term(c, lambda, rows_of(nd));
      stack.assign(1, nd);
      while (!stack.empty()) {
        const int32_t x = stack.back(); stack.pop_back();
        if (x < n) { row_cluster[x] = c; row_lambda[x] = lambda; }
        else { stack.push_back(h.left[x - n]); stack.push_back(h.right[x - n]); }
      }
    };
    auto new_cluster = [&](int32_t nd, int32_t c, double lambda) {
      const int32_t id = (int32_t)parent.size();
      parent.push_back(c); child_a.push_back(-1); child_b.push_back(-1);
      birth.push_back(lambda); stability.push_back(0.0); lambda_max.push_back(0.0);
      term(c, lambda, rows_of(nd));
      cluster_of[nd - n] = id;                                          // rows_of(nd) >= min_cluster_size >= 2: an internal node
      return id;
    };
    for (int64_t k = m - 1; k >= 0; --k) {
      const int32_t c = cluster_of[k];
      if (c < 0) continue;
      const int32_t l = h.left[k], r = h.right[k];
      const double lambda = ew[k] > 0.0 ? 1.0 / ew[k] : inf;
      const bool big_l = rows_of(l) >= min_cluster_size, big_r = rows_of(r) >= min_cluster_size;
      if (big_l && big_r) {
        const int32_t a = new_cluster(l, c, lambda);
        const int32_t b = new_cluster(r, c, lambda);
        child_a[c] = a; child_b[c] = b;
      } else {
        if (big_l) cluster_of[l - n] = c; else fall_out(l, c, lambda);
        if (big_r) cluster_of[r - n] = c; else fall_out(r, c, lambda);
      }
    }
    // ---- excess of mass, bottom-up; then nothing under a selected cluster stays selected
    const int32_t nc = (int32_t)parent.size();
    std::vector<char> selected(nc, 1);
    selected[0] = 0;
    for (int32_t c = nc - 1; c >= 1; --c) {
      if (child_a[c] < 0) continue;
      const double s = stability[child_a[c]] + stability[child_b[c]];
      if (s > stability[c]) { selected[c] = 0; stability[c] = s; }
    }
    std::vector<int32_t> owner(nc, -1);                                 // the selected cluster a cluster is, or lies under
    for (int32_t c = 1; c < nc; ++c) owner[c] = owner[parent[c]] >= 0 ? owner[parent[c]] : (selected[c] ? c : -1);
    // ---- labels, numbered by smallest member row; probabilities
    std::vector<int32_t> number(nc, -1);
    int32_t made = 0;
    for (int64_t i = 0; i < n; ++i) {
      const int32_t c = owner[row_cluster[i]];
      if (c < 0) { labels[i] = -1; prob[i] = 0.0; continue; }
      if (number[c] < 0) number[c] = made++;
      labels[i] = number[c];
      const double top = lambda_max[c], lam = row_lambda[i] < top ? row_lambda[i] : top;
      const double q = lam / top;
      prob[i] = std::isfinite(q) ? q : 1.0;
    }
    *n_clusters = made;
  } catch (const std::bad_alloc&) {
    return GR_ERR_STATE;
  }
  return GR_OK;
}
