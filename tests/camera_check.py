"""The comparison the camera's GPU tests share: one image of the device against its fp64 brute-force reference
(camera_ref.reference_image, camera_drones_ref.reference_image)."""
import numpy as np

from tests import camera_drones_ref as dr
from tests import camera_ref as cr


def check_image(k, dep, seg, ref, L, metric, far=1000.0, tol=cr.KERNEL_TOL, sphere_tol=dr.SPHERE_TOL):
    """One camera's image against its reference.  The reference's ambiguity mask is at most 1 % of the image (a condition: a mask
    that grows cannot hide a failure); outside it hit / no-hit and seg are equal and |t - t_ref| <= tol t_ref / max(|n . d|, 0.05),
    tol = `sphere_tol` where a sphere wins (ref["is_drone"], when the reference has drones) and `tol` elsewhere.  A depth-buffer
    image (metric False) is mapped back to t and granted 3 ulp of 1.0 of the stored value on top.  Prints and returns the worst
    |dt| / bound (<= 1 passes; 0.0 where nothing is hit)."""
    amb = ref["ambiguous"]
    assert amb.mean() <= 0.01, (k, amb.mean())
    ok = ~amb
    dep = dep.astype(np.float64)
    t = dep if metric else cr.depth_buffer_to_t(dep, float(np.float32(L)), far)
    hit_ref = np.isfinite(ref["t"])
    assert np.array_equal(np.isfinite(t)[ok], hit_ref[ok]), (k, int((np.isfinite(t) != hit_ref)[ok].sum()))
    if not metric:
        assert (dep[ok & ~hit_ref] == 1.0).all()
    if seg is not None:
        assert np.array_equal(seg[ok], ref["seg"][ok]), (k, int((seg != ref["seg"])[ok].sum()))
    m = ok & hit_ref
    if not m.any():
        return 0.0
    tr, nd = ref["t"][m], np.maximum(ref["ndot"][m], 0.05)
    on_drone = ref["is_drone"][m] if "is_drone" in ref else np.zeros(tr.shape, bool)
    bound = np.where(on_drone, sphere_tol, tol) * tr / nd
    if not metric:
        near = float(np.float32(L))
        bound = bound + 3.0 * 2.0 ** -24 * tr * tr * (far - near) / (far * near)
    ratio = np.abs(t[m] - tr) / bound
    drones = f" ({int(on_drone.sum())} on drones)" if "is_drone" in ref else ""
    print(f"  camera {k}: {int(m.sum())} hits{drones}, ambiguous {100 * amb.mean():.3f} %, worst |dt| / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0, (k, float(ratio.max()))
    return float(ratio.max())
