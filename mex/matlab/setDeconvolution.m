function setDeconvolution(r, sigma, iterations, floorValue)
% setDeconvolution  Richardson-Lucy deconvolution of the emission volume on the device, without uploading it again.
% (Untested: written without access to MATLAB; the command it sends is tested through the mex stub.)
%
%   setDeconvolution(r, [1 1 2], 10)        % Gaussian PSF, sigma in voxels per dimension of Data, 10 iterations
%   setDeconvolution(r, 1.5, 20, 1e-5)      % one sigma for all three dimensions, another floor
%   setDeconvolution(r, [])                 % none: the unmodified volume again
%
% The emission volume on the device becomes what deconvlucy(max(Data, 0), psf, iterations) computes for a
% separable Gaussian psf of size 2*ceil(2*sigma)+1 with replicate padding, in single precision with this
% library's own order of operations: per iteration the estimate is blurred, Data is divided by the larger
% of the blur and the floor (default 1e-6), the ratio is blurred with the same filter and multiplies the
% estimate.  sigma is at most 6, iterations at most 64; a dimension with sigma 0, or of length 1, is not
% filtered.  The setting stays with the object's handle: every later render, renderProjection,
% renderIsosurface, renderTransfer, renderSlice, volumeHistogram and renderChannels sees the deconvolved
% volume, also after the next upload; smoothing (setSmoothing) and label gains (setLabelGains) apply to
% the deconvolved voxels.  A VolumeAbsorption that is the same Volume as VolumeEmission follows; gradient
% volumes of lookup mode are not recomputed.  Handles that span several GPUs (VR_DEVICES) refuse it.
% (volumeRender('set_deconvolution', h, sigma, iterations, floor); vr_set_deconvolution in include/vrhip.h.)
if isempty(sigma) || nargin < 3 || isequal(iterations, 0)
    volumeRender('set_deconvolution', r.objectHandle, []);
    return;
end
if ~isnumeric(sigma) || ~(isscalar(sigma) || (isvector(sigma) && numel(sigma) == 3))
    error('sigma must be a scalar or a vector of 3 values.');
end
if ~isnumeric(iterations) || ~isscalar(iterations) || iterations ~= round(iterations)
    error('iterations must be an integer scalar.');
end
if nargin < 4
    volumeRender('set_deconvolution', r.objectHandle, single(sigma(:)'), double(iterations));
else
    volumeRender('set_deconvolution', r.objectHandle, single(sigma(:)'), double(iterations), single(floorValue));
end
end
