function [image, depth, normal] = renderIsosurface(r, level)
% renderIsosurface  The first-hit isosurface of the emission volume through the current camera.
%
%   image                  = renderIsosurface(r, level)
%   [image, depth, normal] = renderIsosurface(r, level)   % r: a VolumeRender with CameraXOffset == 0
%
% NOT TESTED: no MATLAB was available when this file was written.  The command underneath
% (volumeRender('render_isosurface', ...)) is tested through the MEX adaptor's test build.
%
% The rays are exactly those of r.render(): the same camera, image resolution, element size and
% step, so the surface lines up pixel for pixel with the rendered frame.  A ray stops at its first
% sample whose emission value is >= level; six bisection steps between that sample and the one before
% place the surface point.  There the lights of r.LightSources shade it through r.VolumeIllumination
% exactly as render() shades a sample (FactorReflection, VolumeReflection, the gradient volumes if
% set), and FactorEmission * value * Color is added.  FactorAbsorption and OpacityThreshold are
% ignored.
%   image   single [H W 3]; 0 where no sample reaches the level
%   depth   single [H W]: the distance from the eye to the surface point, NaN without a surface
%   normal  single [H W 3]: the unit normal -gradient / |gradient|, NaN without a surface (and on a
%           zero gradient)
% (vr_render_isosurface in include/vrhip.h states the arithmetic.)
%
% With CameraXOffset ~= 0 the two eyes are rendered at +-base and combined by r.StereoOutput exactly
% as VolumeRender.render combines its two renders (VolumeRender.m:278-307); a stereo isosurface has
% no depth or normal plane.
if ~(isnumeric(level) && isreal(level) && isscalar(level))
    error('level must be a real scalar');
end
if all([islogical(r.VolumeReflection), islogical(r.VolumeAbsorption), islogical(r.VolumeEmission)])
    error('Not all volumes are properly set!');
end
if r.CameraXOffset == 0
    [image, depth, normal] = surface(r, single(0), flip(r.ImageResolution), level);
    return;
end
if nargout > 1
    error('A stereo isosurface returns no depth or normal plane.');
end
base = r.CameraXOffset / 2;
fov = 2 * atan(1 / r.FocalLength);
delta = round((base * r.ImageResolution(2)) / (2 * r.FocalLength * tan(fov / 2)));
resolution = flip(r.ImageResolution) + [0, delta];
rightImage = surface(r, base, resolution, level);
leftImage = surface(r, -base, resolution, level);
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

function [image, depth, normal] = surface(r, cameraXOffset, resolution, level)
% one 'render_isosurface' call: the volumes synced as p_render syncs them, the nine 'render'
% arguments (the lights and the LUT are uploaded as 'render' uploads them), then the level
r.syncVolumes();
factors = single([r.FactorEmission, r.FactorReflection, r.FactorAbsorption]);
props = single([cameraXOffset, r.FocalLength, r.DistanceToObject]);
[image, depth, normal] = volumeRender('render_isosurface', r.objectHandle, r.LightSources, ...
    r.VolumeIllumination, factors, single(r.ElementSizeUm), uint64(resolution), ...
    single(flip(r.RotationMatrix)), props, single(r.OpacityThreshold), single(r.Color), single(level));
end
