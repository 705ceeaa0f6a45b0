function [S, Y, convergence_error, state] = proposed_algorithm_resume_f64(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S, state, it0)
% basic_system_functions/proposed_algorithm.m (with indx_S: proposed_algorithm_angles.m), type 'approximate' or 'std', in float64
% on the MI355X, resumed from a saved state (jstsp_proposed_resume_f64 / jstsp_proposed_std_resume_f64): iterations
% it0+1 ... it0+Imax of the reference loop.  state: (4*N*M + 2*Gr*G2) x batch complex, the columns [X(:); V1(:); V2(:); C(:); v; S(:)]
% of the problems, or [] = from zero (it0 = 0; the result of proposed_algorithm_f64 / proposed_algorithm_std_f64).  The fourth
% output is the state after the last iteration: hand it to the next call, with it0 advanced by Imax, and the legs return what one
% call of all the iterations returns.  convergence_error holds the rows of the iterations this call ran.
  if nargin < 10, indx_S = []; end
  if nargin < 11, state = []; end
  if nargin < 12, it0 = 0; end
  if nargout >= 4
    [S, Y, convergence_error, state] = jstsp_mex('proposed_algorithm_resume_f64', subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S, state, it0);
  elseif nargout == 3
    [S, Y, convergence_error] = jstsp_mex('proposed_algorithm_resume_f64', subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S, state, it0);
  elseif nargout == 2
    [S, Y] = jstsp_mex('proposed_algorithm_resume_f64', subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S, state, it0);
  else
    S = jstsp_mex('proposed_algorithm_resume_f64', subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S, state, it0);
  end
end
