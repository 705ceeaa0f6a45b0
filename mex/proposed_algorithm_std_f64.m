function [S, Y, convergence_error, rcond] = proposed_algorithm_std_f64(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S, PA, PB)
% Alg. 1 - basic_system_functions/proposed_algorithm.m with type 'std' (and, with indx_S, proposed_algorithm_angles.m) -
% evaluated in float64 on the MI355X (jstsp_proposed_std_f64): v = U\(L\k) as pinv(A)*K*pinv(B), nothing narrowed.
% indx_S, PA, PB are optional ([] = not given): PA = pinv(A), PB = pinv(B), e.g. from pinv_f64, paged as A and B are; a factor
% that is given is not inverted again, so several calls on the same dictionaries share one inversion.
% rcond: [rcond over the A factors, over the B factors] the call inverted itself, NaN for a side that was given.
  if nargin < 10, indx_S = []; end
  if nargin < 11, PA = []; end
  if nargin < 12, PB = []; end
  if nargout >= 4
    [S, Y, convergence_error, rcond] = jstsp_mex('proposed_algorithm_std_f64', subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S, PA, PB);
  elseif nargout == 3
    [S, Y, convergence_error] = jstsp_mex('proposed_algorithm_std_f64', subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S, PA, PB);
  elseif nargout == 2
    [S, Y] = jstsp_mex('proposed_algorithm_std_f64', subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S, PA, PB);
  else
    S = jstsp_mex('proposed_algorithm_std_f64', subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S, PA, PB);
  end
end
