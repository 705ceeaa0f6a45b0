function [Z, support, count] = mmv_omp_f64(A, K, Y, pnorm)
% Joint (MMV) OMP in float64 on the MI355X (jstsp_mmv_omp_f64): the "OMP with MMV" column of plot_errorVSsnr.m:116-117
% with residual, basis, row scores, least squares and Z in double - nothing is narrowed.  The pages of Y are independent
% problems; a 2-D A is shared by them.  pnorm: 2 (default, Chen-Huo) or 1 (Tropp's S-OMP).
% support: K x pages int32, 1-based atoms in selection order, 0 beyond count; count: pages x 1 int32.
  if nargin < 4
    pnorm = 2;
  end
  if nargout >= 3
    [Z, support, count] = jstsp_mex('mmv_omp_f64', A, K, Y, pnorm);
  elseif nargout == 2
    [Z, support] = jstsp_mex('mmv_omp_f64', A, K, Y, pnorm);
  else
    Z = jstsp_mex('mmv_omp_f64', A, K, Y, pnorm);
  end
end
