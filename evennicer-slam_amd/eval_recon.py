"""Reconstruction metrics of the reference's src/tools/eval_recon.py:24-43 (meshes or point sets against ground-truth
surface points), with scipy.spatial.cKDTree.  Distances are in the units of the points (metres for the reference)."""
import numpy as np
from scipy.spatial import cKDTree as KDTree


def completion_ratio(gt_points, rec_points, dist_th=0.05):
    """Fraction of the ground-truth points within dist_th of a reconstructed point."""
    distances, _ = KDTree(rec_points).query(gt_points)
    return float(np.mean((distances < dist_th).astype(np.float64)))


def accuracy(gt_points, rec_points):
    """Mean distance of the reconstructed points to the ground truth."""
    distances, _ = KDTree(gt_points).query(rec_points)
    return float(np.mean(distances))


def completion(gt_points, rec_points):
    """Mean distance of the ground-truth points to the reconstruction."""
    distances, _ = KDTree(rec_points).query(gt_points)
    return float(np.mean(distances))
