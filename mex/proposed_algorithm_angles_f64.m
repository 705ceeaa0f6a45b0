function [S, Y, convergence_error] = proposed_algorithm_angles_f64(subY, Omega, indx_S, A, B, Imax, tau_Y, tau_S, rho, type, greedy_nnz)
% basic_system_functions/proposed_algorithm_angles.m (same signature, type 'approximate') in float64 on the MI355X
% (jstsp_proposed_algorithm_f64 with indx_S); greedy_nnz is unused there too.
  if nargout >= 3
    [S, Y, convergence_error] = jstsp_mex('proposed_algorithm_f64', subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S);
  elseif nargout == 2
    [S, Y] = jstsp_mex('proposed_algorithm_f64', subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S);
  else
    S = jstsp_mex('proposed_algorithm_f64', subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S);
  end
end
