//! Drop-in for src/clustering.rs of dkohlsdorf/audio_pattern_discovery: Merge, ClusteringOperation and the two associated
//! functions main.rs calls (clustering.rs:8-25, 40-76, 81-110), bodies on the MI355X.  UNCOMPILED (no Rust toolchain here).
//!
//! NOT carried over: `pub fn merge(&mut self) -> ClusteringOperation` (clustering.rs:175-209) and the struct's state it steps
//! (`parents`, `distances`, `n_instances`: clustering.rs:27-33).  It is `pub` in the reference but called from exactly one place,
//! the loop inside `clustering` (clustering.rs:104-107); on the GPU that loop runs device-side (three launches per merge, replayed as
//! a hipGraph) and a host-visible single step would mean a synchronisation and a state download per merge.  A caller that
//! wants the dendrogram one merge at a time reads the returned `Vec<ClusteringOperation>` in order: entry t IS what the t-th `merge()`
//! call returns.
use crate::apd_sys::*;
use std::collections::HashSet;

/// clustering.rs:8-13
#[derive(Debug)]
pub enum Merge {
    Sequence2Sequence,
    Sequence2Cluster,
    Cluster2Sequence,
    Cluster2Cluster,
}

/// clustering.rs:19-25 (`distance` private, as there)
#[derive(Debug)]
pub struct ClusteringOperation {
    pub merge_i: usize,
    pub merge_j: usize,
    pub into: usize,
    distance: f32,
    pub operation: Merge,
}

impl ClusteringOperation {
    fn to_c(&self) -> apd_cluster_op {
        apd_cluster_op { merge_i: self.merge_i as u32, merge_j: self.merge_j as u32, into: self.into as u32, distance: self.distance,
                         operation: match self.operation { Merge::Sequence2Sequence => 0, Merge::Sequence2Cluster => 1,
                                                           Merge::Cluster2Sequence => 2, Merge::Cluster2Cluster => 3 } }
    }
}

/// The reference keeps parents / distances / counters here (clustering.rs:31-37); on the GPU that state lives in HBM for the
/// duration of `clustering`, so the type only carries the associated functions.
pub struct AgglomerativeClustering;

fn with_context<T>(f: impl FnOnce(*mut apd_context) -> T) -> T {
    let device = std::env::var("APD_DEVICES").ok().and_then(|s| s.split(',').next().and_then(|t| t.trim().parse().ok())).unwrap_or(0);
    let mut ctx = std::ptr::null_mut();
    unsafe { check(apd_create(device, &mut ctx)); }
    let out = f(ctx);
    unsafe { apd_destroy(ctx); }
    out
}

impl AgglomerativeClustering {
    /// clustering.rs:81-110: percentile threshold over all n*n values, then average-linkage merges until a linkage reaches
    /// it (that merge is still emitted).  Exact linkage ties take the lowest (merge_i, merge_j); the reference iterates a
    /// HashSet there (clustering.rs:180-181), i.e. no order of its own.
    pub fn clustering(distances: Vec<f32>, n_instances: usize, perc: f32) -> (Vec<ClusteringOperation>, HashSet<usize>) {
        let mut ops = vec![apd_cluster_op::default(); n_instances.max(1)];
        let mut roots = vec![0u32; n_instances.max(1)];
        let (mut n_ops, mut n_roots, mut threshold) = (0u32, 0u32, 0f32);
        with_context(|ctx| unsafe {
            check(apd_clustering(ctx, distances.as_ptr(), 0, n_instances as u32, perc, ops.as_mut_ptr(), &mut n_ops,
                                 roots.as_mut_ptr(), &mut n_roots, &mut threshold));
        });
        println!("Clustering with {}", threshold);                                  // clustering.rs:102
        let ops = ops[..n_ops as usize].iter().map(|o| ClusteringOperation {
            merge_i: o.merge_i as usize, merge_j: o.merge_j as usize, into: o.into as usize, distance: o.distance,
            operation: match o.operation { 0 => Merge::Sequence2Sequence, 1 => Merge::Sequence2Cluster,
                                           2 => Merge::Cluster2Sequence, _ => Merge::Cluster2Cluster },
        }).collect();
        (ops, roots[..n_roots as usize].iter().map(|r| *r as usize).collect())
    }

    /// Not in the reference: the linkage of clustering.rs:153-170 between every query (a cluster of its own) and every set of corpus
    /// sequence numbers in `sets` (as cluster_sets returns them), from the cross matrices of alignments::align_cross.  Returns, per
    /// query, the set merge() would pick (None if no linkage is below +INF) and that linkage.
    pub fn cross_linkage(fs: &[f32], sf: &[f32], n_queries: usize, n_corpus: usize, sets: &[Vec<usize>]) -> Vec<(Option<usize>, f32)> {
        let members: Vec<u32> = sets.iter().flat_map(|s| s.iter().map(|v| *v as u32)).collect();
        let mut set_off = vec![0u32; sets.len() + 1];
        for (k, s) in sets.iter().enumerate() { set_off[k + 1] = set_off[k] + s.len() as u32; }
        let mut nearest = vec![0u32; n_queries.max(1)];
        let mut linkage = vec![0f32; n_queries.max(1)];
        with_context(|ctx| unsafe {
            check(apd_cross_linkage(ctx, fs.as_ptr(), sf.as_ptr(), 0, n_queries as u32, n_corpus as u32, members.as_ptr(), set_off.as_ptr(),
                                    sets.len() as u32, std::ptr::null_mut(), std::ptr::null_mut(), nearest.as_mut_ptr(), linkage.as_mut_ptr()));
        });
        (0..n_queries).map(|q| (if nearest[q] == u32::MAX { None } else { Some(nearest[q] as usize) }, linkage[q])).collect()
    }

    /// Not in the reference: the medoid of every set of `sets` (as cluster_sets returns them) from the n x n matrix of align_all
    /// (apd_cluster_medoids): per set the member whose summed distances to and from the members (ascending, one f32 add per term)
    /// are smallest, the smallest sequence number among equals, and that cost; None with an infinite cost for an empty set or one
    /// whose costs are all +INF / NaN.
    pub fn medoids(distances: &[f32], n_instances: usize, sets: &[Vec<usize>]) -> Vec<(Option<usize>, f32)> {
        let members: Vec<u32> = sets.iter().flat_map(|s| s.iter().map(|v| *v as u32)).collect();
        let mut set_off = vec![0u32; sets.len() + 1];
        for (k, s) in sets.iter().enumerate() { set_off[k + 1] = set_off[k] + s.len() as u32; }
        let mut medoid = vec![0u32; sets.len().max(1)];
        let mut cost = vec![0f32; sets.len().max(1)];
        with_context(|ctx| unsafe {
            check(apd_cluster_medoids(ctx, distances.as_ptr(), 0, n_instances as u32, members.as_ptr(), set_off.as_ptr(), sets.len() as u32,
                                      medoid.as_mut_ptr(), cost.as_mut_ptr()));
        });
        (0..sets.len()).map(|k| (if medoid[k] == u32::MAX { None } else { Some(medoid[k] as usize) }, cost[k])).collect()
    }

    /// Not in the reference: the k nearest entries of every row (`by_columns` false: query q ranks distances[q][..]) or column
    /// (true: distances[..][q]) of a rows x cols matrix of align_all or align_cross (apd_neighbors), ascending by (value, index),
    /// NaN entries dropped and, with `skip_self`, entry q itself.  Per query the (index, distance) pairs found: at most k.
    pub fn neighbors(distances: &[f32], rows: usize, cols: usize, k: usize, by_columns: bool, skip_self: bool) -> Vec<Vec<(usize, f32)>> {
        let n_queries = if by_columns { cols } else { rows };
        let mut index = vec![0u32; (n_queries * k).max(1)];
        let mut distance = vec![0f32; (n_queries * k).max(1)];
        let mut count = vec![0u32; n_queries.max(1)];
        with_context(|ctx| unsafe {
            check(apd_neighbors(ctx, distances.as_ptr(), 0, rows as u32, cols as u32, if by_columns { APD_NEIGHBORS_COLUMNS } else { APD_NEIGHBORS_ROWS },
                                std::ptr::null(), 0, k as u32, skip_self as i32, index.as_mut_ptr(), distance.as_mut_ptr(), count.as_mut_ptr(),
                                std::ptr::null_mut()));
        });
        (0..n_queries).map(|q| (0..count[q] as usize).map(|s| (index[q * k + s] as usize, distance[q * k + s])).collect()).collect()
    }

    /// Not in the reference: the prefix of `operations` a run at `threshold` performs (apd_dendrogram_cut: the loop condition of
    /// clustering.rs:104-108 replayed; the operation that reaches the threshold is kept).
    pub fn dendrogram_cut(operations: &[ClusteringOperation], threshold: f32) -> &[ClusteringOperation] {
        let ops: Vec<apd_cluster_op> = operations.iter().map(|o| o.to_c()).collect();
        let mut n_kept = 0u32;
        unsafe { check(apd_dendrogram_cut(ops.as_ptr(), ops.len() as u32, threshold, &mut n_kept)); }
        &operations[..n_kept as usize]
    }

    /// clustering.rs:115-128 (private there) after the merges of `operations`: every instance's root, singletons their own number
    /// (apd_cut_labels).  Panics on a list that is not a dendrogram over n_instances.
    pub fn assignment(operations: &[ClusteringOperation], n_instances: usize) -> Vec<usize> {
        let ops: Vec<apd_cluster_op> = operations.iter().map(|o| o.to_c()).collect();
        let mut labels = vec![0u32; n_instances.max(1)];
        unsafe { check(apd_cut_labels(ops.as_ptr(), ops.len() as u32, n_instances as u32, labels.as_mut_ptr())); }
        labels[..n_instances].iter().map(|l| *l as usize).collect()
    }

    /// Not in the reference: the silhouette of every assignment in `labels` (n_instances labels each, as `assignment` returns them)
    /// over the n x n matrix of align_all (apd_silhouette); `by_columns` false: dist(i, y) = distances[i][y], true: distances[y][i].
    /// Per assignment (score, distinct labels, instances whose silhouette is NaN).
    pub fn silhouette(distances: &[f32], n_instances: usize, labels: &[Vec<usize>], by_columns: bool) -> Vec<(f32, usize, usize)> {
        let flat: Vec<u32> = labels.iter().flat_map(|l| l.iter().map(|v| *v as u32)).collect();
        let cuts = labels.len();
        let mut score = vec![0f32; cuts.max(1)];
        let mut clusters = vec![0u32; cuts.max(1)];
        let mut nans = vec![0u32; cuts.max(1)];
        with_context(|ctx| unsafe {
            check(apd_silhouette(ctx, distances.as_ptr(), 0, n_instances as u32, if by_columns { APD_NEIGHBORS_COLUMNS } else { APD_NEIGHBORS_ROWS },
                                 flat.as_ptr(), cuts as u32, score.as_mut_ptr(), clusters.as_mut_ptr(), nans.as_mut_ptr(),
                                 std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut()));
        });
        (0..cuts).map(|c| (score[c], clusters[c] as usize, nans[c] as usize)).collect()
    }

    /// Not in the reference: DBSCAN over the n x n matrix of align_all for every (eps, min_pts) of `settings`, at most
    /// APD_DENSITY_MAX_SETTINGS of them, in one pass over the matrix (apd_density_clusters).  `both` false: i and j are neighbours when
    /// distances[i][j] <= eps or distances[j][i] <= eps, true: when both are.  Per setting (labels, kind, [clusters, core, border,
    /// noise]): a core point's label is the smallest core point of its component, a border point's the smallest label among its core
    /// neighbours, a noise point's its own number -- what `silhouette` takes; kind is APD_DENSITY_NOISE, _BORDER or _CORE.
    pub fn density(distances: &[f32], n_instances: usize, settings: &[(f32, usize)], both: bool) -> Vec<(Vec<usize>, Vec<u8>, [usize; 4])> {
        let eps: Vec<f32> = settings.iter().map(|s| s.0).collect();
        let min_pts: Vec<u32> = settings.iter().map(|s| s.1 as u32).collect();
        let count = settings.len();
        let mut labels = vec![0u32; (count * n_instances).max(1)];
        let mut kind = vec![0u8; (count * n_instances).max(1)];
        let mut counts = vec![0u32; (count * 4).max(1)];
        with_context(|ctx| unsafe {
            check(apd_density_clusters(ctx, distances.as_ptr(), 0, n_instances as u32, if both { APD_DENSITY_BOTH } else { APD_DENSITY_EITHER },
                                       eps.as_ptr(), min_pts.as_ptr(), count as u32, labels.as_mut_ptr(), kind.as_mut_ptr(), std::ptr::null_mut(),
                                       counts.as_mut_ptr(), std::ptr::null_mut()));
        });
        (0..count).map(|s| (labels[s * n_instances..(s + 1) * n_instances].iter().map(|l| *l as usize).collect(),
                            kind[s * n_instances..(s + 1) * n_instances].to_vec(),
                            [counts[4 * s] as usize, counts[4 * s + 1] as usize, counts[4 * s + 2] as usize, counts[4 * s + 3] as usize])).collect()
    }

    /// Not in the reference: the density hierarchy of the n x n matrix of align_all at one min_pts (apd_density_tree): every eps of
    /// `density` at once.  (core, edges): core[i] is the (min_pts - 1)-th smallest symmetrised distance of i (-INF for min_pts = 1,
    /// NaN when missing), so core[i] <= eps exactly when `density` calls i core; edges are the (i, j, weight) of the minimum
    /// spanning forest of the mutual reachability, i < j, ascending by (weight, i, j).  With min_pts = 1: single linkage.
    /// Like the rest of this module it has not been compiled (no rustc where it was written).
    pub fn density_tree(distances: &[f32], n_instances: usize, min_pts: usize, both: bool) -> (Vec<f32>, Vec<(usize, usize, f32)>) {
        let slots = n_instances.saturating_sub(1).max(1);
        let mut core = vec![0f32; n_instances.max(1)];
        let (mut edge_i, mut edge_j, mut weight) = (vec![0u32; slots], vec![0u32; slots], vec![0f32; slots]);
        let (mut n_edges, mut nans) = (0u32, 0u64);
        with_context(|ctx| unsafe {
            check(apd_density_tree(ctx, distances.as_ptr(), 0, n_instances as u32, if both { APD_DENSITY_BOTH } else { APD_DENSITY_EITHER },
                                   min_pts as u32, core.as_mut_ptr(), edge_i.as_mut_ptr(), edge_j.as_mut_ptr(), weight.as_mut_ptr(), &mut n_edges,
                                   &mut nans));
        });
        core.truncate(n_instances);
        (core, (0..n_edges as usize).map(|t| (edge_i[t] as usize, edge_j[t] as usize, weight[t])).collect())
    }

    /// Not in the reference: `density` at every eps of `eps`, read off a `density_tree` on the host (apd_density_tree_cut).  Per eps
    /// (labels, [clusters, core, 0, noise]): a core point's label is the smallest point of its component, every other point keeps
    /// its own number (no border points).  Panics on a NaN eps or an edge list that is not a forest.
    pub fn density_cut(core: &[f32], edges: &[(usize, usize, f32)], eps: &[f32]) -> Vec<(Vec<usize>, [usize; 4])> {
        let n = core.len();
        let edge_i: Vec<u32> = edges.iter().map(|e| e.0 as u32).collect();
        let edge_j: Vec<u32> = edges.iter().map(|e| e.1 as u32).collect();
        let weight: Vec<f32> = edges.iter().map(|e| e.2).collect();
        let mut labels = vec![0u32; (eps.len() * n).max(1)];
        let mut counts = vec![0u32; (eps.len() * 4).max(1)];
        unsafe {
            check(apd_density_tree_cut(n as u32, core.as_ptr(), edge_i.as_ptr(), edge_j.as_ptr(), weight.as_ptr(), edges.len() as u32, eps.as_ptr(),
                                       eps.len() as u32, labels.as_mut_ptr(), std::ptr::null_mut(), counts.as_mut_ptr()));
        }
        (0..eps.len()).map(|s| (labels[s * n..(s + 1) * n].iter().map(|l| *l as usize).collect(),
                                [counts[4 * s] as usize, counts[4 * s + 1] as usize, counts[4 * s + 2] as usize, counts[4 * s + 3] as usize])).collect()
    }

    /// clustering.rs:40-76: leaf lists per root; roots that were never merged are skipped ("Cluster not found").
    pub fn cluster_sets(operations: &[ClusteringOperation], cluster_ids: &HashSet<usize>, n_instances: usize) -> Vec<Vec<usize>> {
        let ops: Vec<apd_cluster_op> = operations.iter().map(|o| o.to_c()).collect();
        let mut roots: Vec<u32> = cluster_ids.iter().map(|r| *r as u32).collect();
        roots.sort();                                                               // the reference walks the HashSet: unspecified order
        let mut members = vec![0u32; n_instances + ops.len() + 2];
        let mut set_off = vec![0u32; roots.len() + 1];
        let mut n_sets = 0u32;
        unsafe {
            check(apd_cluster_sets(ops.as_ptr(), ops.len() as u32, roots.as_ptr(), roots.len() as u32, n_instances as u32,
                                   members.as_mut_ptr(), set_off.as_mut_ptr(), &mut n_sets));
        }
        (0..n_sets as usize).map(|s| members[set_off[s] as usize..set_off[s + 1] as usize].iter().map(|v| *v as usize).collect()).collect()
    }
}
