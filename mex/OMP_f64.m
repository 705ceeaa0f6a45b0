function [x_hat, indexSet, v, targetMatrix] = OMP_f64(A, v, m, snr)
% benchmark_algorithms/OMP.m evaluated in float64 on the MI355X (jstsp_omp_f64): residual, basis, correlations and the
% least squares in double - nothing is narrowed.  Same signature as OMP.m (snr is unused there too); the columns of v
% are independent problems, a 2-D A is shared by them.
  if nargin < 4
    snr = 0;
  end
  [x_hat, indexSet, v, targetMatrix] = jstsp_mex('omp_f64', A, v, m, snr);
end
