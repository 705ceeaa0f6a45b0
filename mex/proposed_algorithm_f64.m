function [S, Y, convergence_error] = proposed_algorithm_f64(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type)
% basic_system_functions/proposed_algorithm.m (same signature, type 'approximate') evaluated in float64 on the
% MI355X (jstsp_proposed_algorithm_f64): nothing is narrowed, unlike proposed_algorithm.m of this directory.
  if nargout >= 3
    [S, Y, convergence_error] = jstsp_mex('proposed_algorithm_f64', subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type);
  elseif nargout == 2
    [S, Y] = jstsp_mex('proposed_algorithm_f64', subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type);
  else
    S = jstsp_mex('proposed_algorithm_f64', subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type);
  end
end
