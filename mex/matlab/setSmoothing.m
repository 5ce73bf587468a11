function setSmoothing(r, sigma)
% setSmoothing  Gaussian smoothing of the emission volume on the device, without uploading it again.
% (Untested: written without access to MATLAB; the command it sends is tested through the mex stub.)
%
%   setSmoothing(r, 1.5)          % sigma in voxels, the same along all three dimensions of Data
%   setSmoothing(r, [1 1 0.4])    % per dimension of VolumeEmission.Data (z spacing usually differs)
%   setSmoothing(r, [])           % none: the unmodified volume again
%
% The emission volume on the device becomes the separable Gaussian of VolumeEmission.Data with the shape
% of imgaussfilt3's defaults -- filter size 2*ceil(2*sigma)+1, replicate padding -- computed in single
% precision; sigma is at most 6.  A dimension with sigma 0, or of length 1, is not filtered.  The sigma
% stays with the object's handle: every later render, renderProjection, renderIsosurface, renderTransfer,
% renderSlice, volumeHistogram and renderChannels sees the smoothed volume, also after the next upload,
% and label gains (setLabelGains) multiply the smoothed voxels.  A VolumeAbsorption that is the same
% Volume as VolumeEmission follows; gradient volumes of lookup mode are not recomputed.  Handles that
% span several GPUs (VR_DEVICES) refuse a smoothing.
% (volumeRender('set_smoothing', h, sigma); vr_set_smoothing in include/vrhip.h.)
if isempty(sigma)
    volumeRender('set_smoothing', r.objectHandle, []);
    return;
end
if ~isnumeric(sigma) || ~(isscalar(sigma) || (isvector(sigma) && numel(sigma) == 3))
    error('sigma must be a scalar or a vector of 3 values.');
end
volumeRender('set_smoothing', r.objectHandle, single(sigma(:)'));
end
