function [image, aux] = renderProjection(r, mode)
% renderProjection  A projection of the emission volume through the current camera.
%
%   image        = renderProjection(r)          % maximum-intensity projection ('mip')
%   image        = renderProjection(r, 'sum')   % ray sum (the "X-ray" view)
%   [image, aux] = renderProjection(r, mode)    % r: a VolumeRender with CameraXOffset == 0
%
% The rays are exactly those of r.render(): the same camera, image resolution, element size and
% step, so a projection lines up pixel for pixel with the rendered frame.  There is no opacity and no
% lighting: every sample of the emission volume along the ray is taken.
%   'mip'  image = FactorEmission * max(sample) * Color; aux is the distance from the eye to the first
%          sample that attains the maximum (NaN where the ray misses the volume) -- the depth a
%          depth-coded MIP is coloured from.
%   'sum'  image = FactorEmission * sum(sample) * step * Color; aux is the ray's sample count n, so
%          the mean projection is image ./ (aux * step) wherever aux > 0.
% The image is single [H W 3], aux single [H W] (volumeRender('render_projection', ...),
% vr_render_projection in include/vrhip.h).
%
% With CameraXOffset ~= 0 the two eyes are projected at +-base and combined by r.StereoOutput exactly
% as VolumeRender.render combines its two renders (VolumeRender.m:278-307); a stereo projection has
% no aux plane.
if nargin < 2
    mode = 'mip';
end
if all([islogical(r.VolumeReflection), islogical(r.VolumeAbsorption), islogical(r.VolumeEmission)])
    error('Not all volumes are properly set!');
end
if r.CameraXOffset == 0
    [image, aux] = project(r, single(0), flip(r.ImageResolution), mode);
    return;
end
if nargout > 1
    error('A stereo projection returns no aux plane.');
end
base = r.CameraXOffset / 2;
fov = 2 * atan(1 / r.FocalLength);
delta = round((base * r.ImageResolution(2)) / (2 * r.FocalLength * tan(fov / 2)));
resolution = flip(r.ImageResolution) + [0, delta];
rightImage = project(r, base, resolution, mode);
leftImage = project(r, -base, resolution, mode);
leftImage = imcrop(leftImage, [(delta + 1) 0 size(leftImage, 2) size(leftImage, 1)]);
rightImage = imcrop(rightImage, [0 0 (size(rightImage, 2) - delta) size(rightImage, 1)]);
if r.StereoOutput == StereoRenderMode.RedCyan
    image = zeros([size(leftImage, 1), size(leftImage, 2), 3]);
    image(:, :, 1) = leftImage(:, :, 1);
    image(:, :, 2) = rightImage(:, :, 2);
    image(:, :, 3) = rightImage(:, :, 3);
else  % StereoRenderMode.LeftRightHorizontal
    image = [leftImage, rightImage];
end
end

function [image, aux] = project(r, cameraXOffset, resolution, mode)
% one 'render_projection' call: the volumes synced as p_render syncs them, the nine 'render' arguments
% (the lights and the LUT are passed for the protocol's sake and ignored), then the mode
r.syncVolumes();
factors = single([r.FactorEmission, r.FactorReflection, r.FactorAbsorption]);
props = single([cameraXOffset, r.FocalLength, r.DistanceToObject]);
[image, aux] = volumeRender('render_projection', r.objectHandle, r.LightSources, ...
    r.VolumeIllumination, factors, single(r.ElementSizeUm), uint64(resolution), ...
    single(flip(r.RotationMatrix)), props, single(r.OpacityThreshold), single(r.Color), mode);
end
