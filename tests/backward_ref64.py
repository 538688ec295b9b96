"""float64 restatement (numpy, no torch) of the trainer's fused BatchNorm / ReLU sweeps: the arithmetic documented in
csrc/fused.h and csrc/fused.hip (bn_apply_bypass, bn_relu_bwd), written once more with nothing fused and nothing reordered.

Every result comes with a MAGNITUDE: the sum of the absolute values of every term that enters it -- through the column sums temp
and vdm too, whose own terms count, not their cancelled values.  A float32 implementation
is held to  |got - ref64| <= K * 2^-24 * mag  ("scaled error" <= K), per element -- a bar that does not loosen where a value
is the small difference of large terms, and does not let a wrong small element hide behind the norm of a matrix.

The bars K are NOT taken from the kernels.  tests/test_backward_ref64.py measures the largest scaled error the float32 C
reference (oracle_batchnorm_backprop, the ReLU mask, oracle_relu_repair, chained) shows against this file on the shapes the
GPU test uses, and K is four times that, at least 8:
  * a d_aff element passes six float32 roundings (dz * mask, + temp, * scale, x - mean, * scale, * vdm, the sum), and the
    forward memo's mean and scale are float32 where this file recomputes them in float64 (var = uvar - mean^2 of two rounded
    values: about (uvar + mean^2) / (var + eps) / 2 ulps of the scale, 1 to 3 for ReLU outputs);
  * the factor 4: the kernels sum columns in another order than the C loop (four row lanes, row chunks, 32 finalize lanes)
    and contract a * b + c to FMAs -- both legitimate, a few ulps each.
"""
import numpy as np

EPS24 = 2.0 ** -24

# quantity -> K (see the module docstring).  The measured float32-oracle maxima these come from are printed, and 4 x each is
# asserted to stay within its K, by tests/test_backward_ref64.py::test_oracle_chain_scaled_errors_give_the_gpu_bars; the numbers
# are recorded in docs/experiments.md.
# Measured oracle maxima: d_aff 1.63, forward 2.54, oderiv_sumsq 1.40, colsum 0.80, value_sum 0.00 (the oracle sums in double).
K = dict(d_aff=8.0, colsum=8.0, value_sum=8.0, oderiv_sumsq=8.0, forward=11.0)


def scaled_error(got, ref, mag):
    """|got - ref| / (2^-24 mag), elementwise; 0 where both the difference and the magnitude are 0."""
    got, ref, mag = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    diff = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = diff / (EPS24 * mag)
    return np.where(diff == 0, 0.0, e)


def bn_columns64(x, eps=1e-3, target_rms=1.0):
    """BatchNormComponent::Propagate's column parameters (nnet-normalize-component.cc:421-452): mean, variance (biased, floored at
    0) and scale = target_rms / sqrt(var + eps) per column."""
    x = np.asarray(x, np.float64)
    mean = x.mean(0)
    var = np.maximum((x * x).mean(0) - mean * mean, 0.0)
    return mean, var, target_rms / np.sqrt(var + eps)


def bn_columns_test64(stats_block, eps=1e-3, target_rms=1.0):
    """The same from stored statistics (BatchNormTestComponent, ComputeDerived :682-715): stats_block = [count, sum[D], sumsq[D]] as
    net.get_stats() returns a BatchNorm's block."""
    st = np.asarray(stats_block, np.float64)
    D = (len(st) - 1) // 2
    mean = st[1:1 + D] / st[0]
    var = np.maximum(st[1 + D:1 + 2 * D] / st[0] - mean * mean, 0.0)
    return mean, var, target_rms / np.sqrt(var + eps)


def scale_cond64(mean, var, eps=1e-3):
    """How much more than its own value enters a column's scale: scale = (uvar - mean^2 + eps)^-1/2 is formed from the DIFFERENCE of
    two stored float32 values (memo rows 1 and 0; in test mode sumsq / count and (sum / count)^2), so to first order a perturbation
    of 2^-24 of each term moves it by 2^-24 scale c, c = (uvar + mean^2 + eps) / (2 (var + eps)).  c is 1 for a centred column and
    grows with mean^2 / var: a ReLU unit that is nearly always on, far from zero, has c in the tens.  The magnitudes below carry a
    factor (1 + c) per factor of scale in a term."""
    mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    return (var + 2.0 * mean * mean + eps) / (2.0 * (var + eps))


def _rows(a, like):
    return np.ones_like(like) if a is None else np.asarray(a, np.float64)


def bn_apply_bypass64(x, mean, scale, mask_rows=None, bypass=0.0, prev_rows=None):
    """out = (x - mean) * scale * mask + bypass * prev (fused.h bn_apply_bypass); mask_rows / prev_rows: one row per row of x, or None."""
    x = np.asarray(x, np.float64)
    out = (x - mean) * scale * _rows(mask_rows, x)
    return out if prev_rows is None else out + float(bypass) * np.asarray(prev_rows, np.float64)


def bn_apply_bypass_mag64(x, mean, scale, mask_rows=None, bypass=0.0, prev_rows=None, cond=0.0):
    """the magnitude of bn_apply_bypass64's result; cond: scale_cond64 of the columns"""
    x = np.asarray(x, np.float64)
    mag = (np.abs(x) + np.abs(mean)) * scale * (1.0 + cond) * np.abs(_rows(mask_rows, x))
    return mag if prev_rows is None else mag + np.abs(float(bypass) * np.asarray(prev_rows, np.float64))


def relu_repair64(deriv_sum, count, self_repair_scale, lower=0.05, upper=0.95):
    """RectifiedLinearComponent::RepairGradients' per-column term (nnet-simple-component.cc:1028-1073, with the 1 / repair_probability
    = 1 / 0.5 of :1062): +scale / 0.5 for a column whose units are on for at most 5 % of the frames counted, -scale / 0.5 for more
    than 95 %, 0 between.  The two comparisons are the reference's own float32 ones (statistics and count cast to float, threshold x count
    rounded to float): a yes / no decision has no more precise restatement, and a column exactly on a threshold is decided by it."""
    ds = np.asarray(deriv_sum, np.float64)
    if self_repair_scale == 0.0 or count == 0.0:
        return np.zeros_like(ds)
    st, c32 = ds.astype(np.float32), np.float32(count)
    v = (st - np.float32(lower) * c32 > 0).astype(np.float64) + (st - np.float32(upper) * c32 > 0).astype(np.float64) - 1.0
    return v * (-float(self_repair_scale) / 0.5)


def bn_relu_bwd64(x, dz, mean, scale, target_rms=1.0, mask_rows=None, test_mode=False, repair=None, cond=0.0):
    """BatchNorm backward (:505-542; test mode :879-922: dX = dZ scale), ReLU backward and the self-repair term, from the ReLU's
    output x (= the BatchNorm's input) and the derivative dz w.r.t. the (masked) BatchNorm output.  repair: relu_repair64's vector or None;
    cond: scale_cond64 of the columns (enters the magnitudes only).
    Returns a dict:
      d_aff, d_aff_mag            derivative w.r.t. the affine output, per element
      colsum, colsum_mag          its column sums (the affine's bias gradient)
      value_sum, value_sum_mag    column sums of x;  deriv_count: count(x > 0) per column (exact)
      oderiv_sumsq, oderiv_mag    column sums of squares of the ReLU's out-derivative dr, by direct summation
      vdm, temp                   memo rows 3 and 4."""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    N = x.shape[0]
    dzm = dz * _rows(mask_rows, x)
    z = (x - mean) * scale
    if test_mode:
        vdm, temp = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    else:
        vdm = (-1.0 / (target_rms * target_rms * N)) * (z * dzm).sum(0) * scale
        temp = -dzm.sum(0) / N
    dr = (dzm + temp) * scale + z * vdm
    # magnitudes: temp and vdm are column sums themselves, so what enters an element through them is every term of those sums --
    # sum |dz m| / N and coeff scale sum (|x| + |mean|) scale |dz m|, not |temp| and |vdm|, which are what is left after the terms
    # cancelled (the heads' derivatives sum to nearly zero over a column: |temp| is 10^-7 of sum |dz| / N there, and a float32 sum is
    # good to 2^-24 of the latter)
    z_mag = (np.abs(x) + np.abs(mean)) * scale
    temp_mag = np.zeros_like(temp) if test_mode else np.abs(dzm).sum(0) / N
    vdm_mag = np.zeros_like(vdm) if test_mode else (1.0 / (target_rms * target_rms * N)) * (z_mag * np.abs(dzm)).sum(0) * scale
    dr_mag = (np.abs(dzm) + temp_mag) * scale * (1.0 + cond) + z_mag * vdm_mag * (1.0 + 3.0 * cond)  # (scale once / three times)
    rep = np.zeros(x.shape[1]) if repair is None else np.asarray(repair, np.float64)
    on = x > 0
    d_aff = on * dr + rep
    d_aff_mag = dr_mag + np.abs(rep)
    return dict(d_aff=d_aff, d_aff_mag=d_aff_mag, colsum=d_aff.sum(0), colsum_mag=np.abs(d_aff).sum(0),
                value_sum=x.sum(0), value_sum_mag=np.abs(x).sum(0), deriv_count=on.sum(0).astype(np.float64),
                oderiv_sumsq=(dr * dr).sum(0), oderiv_mag=(dr_mag * dr_mag).sum(0), vdm=vdm, temp=temp, on=on, repair=rep)
