function setLabelGains(r, gains, labels)
% setLabelGains  Fade segmented regions of the emission volume without uploading it again.
%
%   setLabelGains(r, gains, labels)   % labels: uint8, size(VolumeEmission.Data), one label per voxel
%   setLabelGains(r, gains)           % new gains for the labels already on the device
%   setLabelGains(r, [])              % no gains: the unmodified volume again
%   setLabelGains(r, gains, [])       % drop the labels
%
% gains is a vector of at most 256 finite values: gains(l + 1) is the factor of the voxels labelled l;
% labels beyond numel(gains) keep the factor 1.  The emission volume on the device becomes
%   single(gains(labels + 1)) .* VolumeEmission.Data
% -- bit for bit what examples/example4.m computes on the host with
%   render.VolumeEmission.Data(logical(mask)) = factor(i) * emission_main.Data(logical(mask));
% and uploads before every frame -- but only the gains cross to the GPU.  The labels are sent once
% (pass a RawVolume of uint8 to have its TimeLastUpdate spare a repeated upload) and stay with the
% object's handle, as the gains do; every render method then sees the faded volume: render (mono and
% stereo), renderChannels, renderProjection, renderIsosurface, renderTransfer, with clip planes too.
% A VolumeAbsorption that is the same Volume as VolumeEmission (the default use) fades with it; gradient
% volumes of lookup mode are not recomputed (example4.m does not recompute them either).  Handles that
% span several GPUs (VR_DEVICES) refuse labels.  The movie of example4.m:
%   setLabelGains(r, [1 1], uint8(mask.Data));
%   for i = 1:numel(factor)
%       setLabelGains(r, [1 factor(i)]);
%       frames(:, :, :, i) = r.render();
%   end
% (volumeRender('sync_labels', h, labels) and volumeRender('set_label_gains', h, single(gains));
%  vr_sync_labels and vr_set_label_gains in include/vrhip.h.)
if nargin >= 3
    if isempty(labels)
        volumeRender('sync_labels', r.objectHandle, []);
    elseif isa(labels, 'Volume')
        volumeRender('sync_labels', r.objectHandle, labels);
    else
        if ~isa(labels, 'uint8')
            error('labels must be a uint8 array (or a RawVolume of uint8).');
        end
        volumeRender('sync_labels', r.objectHandle, labels);
    end
end
if isempty(gains)
    volumeRender('set_label_gains', r.objectHandle, []);
    return;
end
if ~isvector(gains) || numel(gains) > 256
    error('gains must be a vector of at most 256 values.');
end
volumeRender('set_label_gains', r.objectHandle, single(gains(:)'));
end
