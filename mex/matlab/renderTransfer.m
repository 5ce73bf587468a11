function [image, alpha] = renderTransfer(r, colormap, clim, alphamap, alim, coord)
% renderTransfer  r.render() with a transfer function: a colormap and an alphamap per sample.
%
%   image          = renderTransfer(r, parula(256))                 % value-coded colour over [0 1]
%   image          = renderTransfer(r, cmap, [lo hi])               % ... over the data range [lo hi]
%   image          = renderTransfer(r, cmap, clim, amap, [lo hi])   % opacity from an alphamap
%   image          = renderTransfer(r, cmap, [tnear tfar], false, [0 1], 'depth')  % depth-coded colour
%   [image, alpha] = renderTransfer(r, ...)                         % r: CameraXOffset == 0
%
% What volshow calls Colormap and Alphamap.  The rays, the step and the compositing are exactly those
% of r.render() (with the exact shading arithmetic); per sample
%   - the emission colour is cmap (N x 3, rows R G B, 2 <= N <= 1024) read at the emission sample
%     mapped from clim = [lo hi] onto the table, linearly interpolated, clamped at both ends --
%     or, with coord = 'depth', at the sample's distance from the eye;
%   - with an alphamap (M values over the absorption-sample range alim) the sample's absorption is
%     FactorAbsorption * amap(absorption sample) instead of FactorAbsorption * absorption sample;
%     false keeps render's opacity.
% r.Color stays the colour of the illumination term.  A constant colormap equal to r.Color and no
% alphamap give the image of r.render().  Changing a map uploads a table of a few KiB, no volume.
% image is single [H W 3], alpha single [H W], the accumulated opacity of each pixel, for compositing
% the channel over something else (volumeRender('render_transfer', ...), vr_render_transfer in
% include/vrhip.h).  Double maps such as parula(256) are cast to single here.
%
% With CameraXOffset ~= 0 the two eyes are rendered at +-base and combined by r.StereoOutput exactly
% as VolumeRender.render combines its two renders (VolumeRender.m:278-307); a stereo render has no
% alpha plane.
%
% (Written against the command's argument list; not run for lack of MATLAB here.)
if nargin < 3 || isempty(clim)
    clim = [0 1];
end
if nargin < 4 || isempty(alphamap)
    alphamap = false;
end
if nargin < 5 || isempty(alim)
    alim = [0 1];
end
if nargin < 6
    coord = 'value';
end
if all([islogical(r.VolumeReflection), islogical(r.VolumeAbsorption), islogical(r.VolumeEmission)])
    error('Not all volumes are properly set!');
end
colormap = single(colormap);
if ~islogical(alphamap)
    alphamap = single(alphamap(:));
end
tf = {colormap, single(clim), alphamap, single(alim), coord};
if r.CameraXOffset == 0
    [image, alpha] = transfer(r, single(0), flip(r.ImageResolution), tf);
    return;
end
if nargout > 1
    error('A stereo transfer render returns no alpha plane.');
end
base = r.CameraXOffset / 2;
fov = 2 * atan(1 / r.FocalLength);
delta = round((base * r.ImageResolution(2)) / (2 * r.FocalLength * tan(fov / 2)));
resolution = flip(r.ImageResolution) + [0, delta];
rightImage = transfer(r, base, resolution, tf);
leftImage = transfer(r, -base, resolution, tf);
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

function [image, alpha] = transfer(r, cameraXOffset, resolution, tf)
% one 'render_transfer' call: the volumes synced as p_render syncs them, the nine 'render' arguments,
% then the transfer function
r.syncVolumes();
factors = single([r.FactorEmission, r.FactorReflection, r.FactorAbsorption]);
props = single([cameraXOffset, r.FocalLength, r.DistanceToObject]);
[image, alpha] = volumeRender('render_transfer', r.objectHandle, r.LightSources, ...
    r.VolumeIllumination, factors, single(r.ElementSizeUm), uint64(resolution), ...
    single(flip(r.RotationMatrix)), props, single(r.OpacityThreshold), single(r.Color), tf{:});
end
